/*
 * golf_amd.h — C ABI of libgolf_hip.so: the MI355X (gfx950) kernels behind GOLF's time-varying
 * LPC synthesis filter and glottal-flow source path.
 *
 * The reference (iamycy/golf) has NO FFI boundary of its own: the arithmetic on this path lives in
 * un-vendored Python/C++/numba packages that its nn.Modules call.  Each entry point below names the
 * reference call site (file:line under /root/reference) whose computation it replaces; the Python
 * binding a maintainer would add is golf_amd/_lib.py (ctypes) — see INTEGRATION.md.
 *
 * Conventions (all entry points)
 *   - plain pointers + sizes only; every pointer is a caller-owned DEVICE buffer (hipMalloc'd or a
 *     torch tensor's data_ptr()), fp32 row-major contiguous unless a stride is given;
 *   - the library never allocates or frees: scratch is passed in as (ws, ws_bytes), sized by the
 *     matching *_workspace_bytes();  ws must be 256-byte aligned;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*), no internal sync,
 *     no global mutable state => re-entrant from several host threads / streams;
 *   - return 0 = ok; <0 = GOLF_E* bad-argument code (text via golf_last_error(), thread-local);
 *     >0 = hipError_t from a launch.
 */
#ifndef GOLF_AMD_H
#define GOLF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOLF_ABI_VERSION 6

enum {
    GOLF_OK = 0,
    GOLF_EINVAL = -1,   /* bad size / null pointer                        */
    GOLF_EWORKSPACE = -2, /* ws too small or misaligned                     */
    GOLF_EUNSUPPORTED = -3 /* shape outside what the kernels cover (message) */
};

int golf_abi_version(void);
const char* golf_last_error(void);
/* "gfx950" — the only code object in the library. */
const char* golf_target_arch(void);

/* ---------------------------------------------------------------------------------------------
 * a-1 (+a-3 fused): sample-wise LTV all-pole filter — GOLF-ss end filter.
 * Replaces LTVMinimumPhaseFilterPrecise.forward, models/filters.py:99-113:
 *     ex*gain (AudioTensor broadcast -> linear upsampling, models/utils.py:538-544)
 *     a.reduce_hop_length() -> (B,T,M) materialised coefficient tensor (never built here)
 *     torchlpc.sample_wise_lpc(ex, a)  (models/filters.py:112)
 *
 *   y[b,t] = ex[b,t]*G[b,t] - sum_{i<M} A[b,t,i]*y[b,t-1-i],  y[<0] = 0,  t in [0,T)
 *   G = up(gain), A = up(a): up(z)[t] = z[f]+(t-f*hop)*(z[f+1]-z[f])/hop, f = min(t/hop, F-2)
 *
 *   ex   (B, >=T) row stride ex_stride      gain (B,F)      a (B,F,M)
 *   y    (B, T)   row stride y_stride       requires 1 <= T <= (F-1)*hop+1, 1 <= M <= 64
 *   ws   scratch of golf_ltv_allpole_workspace_bytes(); it also carries the per-chunk transition
 *        matrices the backward pass reuses — keep it alive (unmodified) until the backward ran.
 *
 *   Two families of kernels serve this entry and the three below.  The RING kernels (time-chunked scan, batch-parallel
 *   serial recursion) need a ring width W in {8,16,24,32,40} with hop % W == 0, M <= W - 2 and F >= 2.  Every other shape
 *   -- any 1 <= M <= 64, hop >= 1, F >= 1: hop 100 / 220 / 300 / 441, orders 39..64, a single frame -- runs on the
 *   WAVE-PER-UTTERANCE kernels (csrc/lpc_any.hip): one wavefront per utterance, one lane per tap, the recursion in scatter
 *   form (a broadcast, a lane shift and an FMA per sample), fp32, 64-bit row addressing (no 2^24 stride limit), about the
 *   time per sample of GOLF_SS_SERIAL whatever the batch size below the chip's wave slots.  For such a shape the forward
 *   needs no workspace (ws may be NULL), the GOLF_SS_SERIAL / _CHUNKED / _FLAT_SCAN bits are ignored, the transitions call
 *   is a no-op and the status words are 0; the backward keeps its intermediate g (B, T) in ws, which
 *   golf_ltv_allpole_workspace_bytes_ex sizes accordingly.
 * ------------------------------------------------------------------------------------------- */
size_t golf_ltv_allpole_workspace_bytes(int B, int T, int F, int M, int hop);
/* The same for a forced algorithm (GOLF_SS_SERIAL / GOLF_SS_CHUNKED in `flags`; 0 = default selection). */
size_t golf_ltv_allpole_workspace_bytes_ex(int B, int T, int F, int M, int hop, int flags);

/* The per-chunk transition matrices depend only on the coefficients `a`, not on the excitation, and are the
 * most expensive phase.  golf_ltv_allpole_transitions_f32 computes them into `ws` on its own, so a caller that
 * knows `a` before `ex` exists can start it early (optionally on a second HIP stream) or reuse it for several
 * excitations, and then pass GOLF_SS_HAVE_TRANSITIONS to the forward.
 *   The transitions call also prepares what the forward's boundary scan derives from the matrices alone (the group
 *   composites of the two-level scan): give BOTH calls the same algorithm flags (GOLF_SS_CHUNKED / _FLAT_SCAN / _FAST_...),
 *   and size `ws` with golf_ltv_allpole_workspace_bytes_ex for those flags.
 *   flags  GOLF_SS_HAVE_TRANSITIONS  `ws` already holds the transitions for (a,B,T,F,M,hop)
 *          GOLF_SS_FAST_TRANSITIONS  inference mode: transition matrices from fp32 instead of fp64 trajectories
 *                (about 4x cheaper) and the forward runs one refinement sweep over the chunk boundary states
 *                (re-run the chunks from the scanned states, rescan with the observed end-state defects), which
 *                makes the result second order in the matrix error: same accuracy as a sequential fp32 recursion.
 *                (ABI 2 required the fp64-derived matrices for the backward; since ABI 3 the backward runs its own refinement
 *                sweep and accepts either: see GOLF_SS_TRAINING.)
 *   side_stream  optional second hipStream_t (may be NULL): without HAVE_TRANSITIONS the forward forks the
 *                transition kernel onto it (event fork/join) so it overlaps the excitation-dependent phase;
 *                with HAVE_TRANSITIONS the forward joins it (event wait) right before the boundary scan. */
#define GOLF_SS_HAVE_TRANSITIONS 1
#define GOLF_SS_FAST_TRANSITIONS 2
/*          GOLF_SS_SPLIT_P1  (diagnostic) launch the fp32 transition kernel and the zero-state pass separately instead
 *                of as one horizontally fused kernel (the default with FAST and without HAVE / side_stream). */
#define GOLF_SS_SPLIT_P1 4
/*          GOLF_SS_SERIAL / GOLF_SS_CHUNKED  force one of the two algorithms (default: by batch size).
 *                CHUNKED: time is cut into chunks whose transition matrices are scanned (B*T/L*(M+2) lanes of work,
 *                (M+2)-fold arithmetic: what makes B = 32 fast).  SERIAL: one quad of lanes per utterance runs the
 *                recursion from t = 0 to T, B/16 waves, no redundant arithmetic and no transition matrices: the
 *                large-batch kernel (default from B >= 2048, where the two meet on MI355X).  The backward must be given the flag the forward ran with. */
#define GOLF_SS_SERIAL 8
#define GOLF_SS_CHUNKED 16
/*          GOLF_SS_FLAT_SCAN  chunk-boundary states by the flat scan (one wave per utterance, NP dependent matvecs)
 *                instead of the two-level scan that long utterances with M <= 24 take by default while the batch is
 *                small (utterances x groups of 16 chunks <= 2 x the CU count: B <= 39 at 2 s; group composites as
 *                f64 MFMA product chains rounded once to fp32 + per-group scans spread over the chip + start states
 *                derived in the chunk kernels): an A/B switch; the two give the same states up to fp32 rounding. */
#define GOLF_SS_FLAT_SCAN 32
/*          GOLF_SS_TRAINING  golf_ltv_allpole_bwd_f32 will follow on this workspace: the forward also keeps what the backward's
 *                two-level adjoint scan reads (the transition matrices in the adjoint's orientation, the group composites
 *                transposed).  Implied without GOLF_SS_FAST_TRANSITIONS.  With FAST | TRAINING the training step runs on the
 *                fp32 transition matrices of the inference path (hot chunks recomputed from fp64 trajectories, one refinement
 *                sweep in the forward AND in the backward): same accuracy class, ~28 us less per B = 32 step (ABI 3). */
#define GOLF_SS_TRAINING 64
/*          GOLF_SS_MAPS_ONLY  (ABI 4, with GOLF_SS_FAST_TRANSITIONS) golf_ltv_allpole_transitions_f32 computes the transition
 *                matrices and nothing else; the forward, given HAVE_TRANSITIONS | MAPS_ONLY, runs what is still missing (the
 *                fix-up of ill-conditioned matrices, the group composites) in the launch that holds its zero-state pass.
 *                The matrices need only `a`: a caller that has the coefficient tracks before the excitation (the decoder: they
 *                come from the encoder, the excitation from the oscillator) issues this call beside the source's launches
 *                (golf_amd.functional.ltv_allpole_prepare(maps_only=True)). */
#define GOLF_SS_MAPS_ONLY 128
/*          GOLF_SS_THROUGHPUT  (ABI 4) the caller keeps SEVERAL batches in flight on the device (a serving loop on a few HIP
 *                streams): prefer the launch structure that costs the least chip time over the one that finishes a lone
 *                batch soonest.  Today: the zero-state pass runs inside the pre-pass launch instead of inside the transition
 *                kernel's, and the two chunk passes are two thin launches instead of the one launch a lone batch gets (whose
 *                waves live through both sweeps, waiting for each other in between) -- one batch alone 123 -> 134 us, four in
 *                flight 75 -> 68.5 us/step, MI355X, B = 32 x 2 s (round 5).  Results are bit-identical either way: the flag changes launches, never
 *                the algorithm.  (The Python host additionally switches an inference forward of >= 512 utterances to GOLF_SS_SERIAL
 *                while it sets this flag -- golf_amd.functional.SS_THROUGHPUT_SERIAL_MIN -- and that IS another algorithm: same
 *                accuracy class, different bits.)  The library cannot see how many batches its
 *                caller keeps in flight, hence a flag (cf. GOLF_SS_SERIAL). */
#define GOLF_SS_THROUGHPUT 256
/*          GOLF_SS_ZERO_TAIL  (ABI 5, golf_ltv_allpole_bwd_f32 only) the excitation rows were longer than the output (the
 *                oscillator renders Tx = 48 000 samples, the filter consumes T = (F-1)*hop + 1 = 47 761): the backward also
 *                writes the zeros that are the gradient of the unused tail, g_ex[b][T .. g_ex_stride), so that the caller
 *                needs neither a full-size memset nor a strided fill launch in front of every backward (each ~5 us of a
 *                ~260 us B = 32 training step).  g_ex must be dense up to its row stride. */
#define GOLF_SS_ZERO_TAIL 512

int golf_ltv_allpole_transitions_f32(const float* a, int B, int T, int F, int M, int hop,
                                     void* ws, size_t ws_bytes, int flags, void* stream);

int golf_ltv_allpole_fwd_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a,
                             float* y, int64_t y_stride, int B, int T, int F, int M, int hop,
                             void* ws, size_t ws_bytes, int flags, void* side_stream, void* stream);

/* Streaming form (additive in ABI 6): the same recursion, up() interpolation and T <= (F-1)*hop+1 rule, but y[<0] is not 0:
 *   y[b][-1-i] = state[b][i],  state (B, M) fp32 DEVICE buffer, in and out (the oracle's `zi`, sample_wise_lpc(x, A, zi)).
 * On return state[b][i] = y[b][T-1-i], the block's last M outputs (for T < M the old state shifted in behind them), so that
 * the next block continues the recursion.  Always a serial recursion (GOLF_SS_SERIAL: 8 or 4 lanes per utterance by batch
 * size; where no ring fits (M, hop, F) the wave-per-utterance kernel, which replays the M state values through its update
 * before the first sample), and the per-tap summation order does not depend on where a block
 * starts: blocks that start on frame boundaries, each given the frames it spans (frame 0 = the frame of its first sample),
 * chained through `state` from zeros, give the same bits as one golf_ltv_allpole_fwd_f32(.., GOLF_SS_SERIAL) over the whole
 * -- on either family of kernels.  No workspace; the row strides must stay below 2^24 on the ring path. */
int golf_ltv_allpole_fwd_state_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a,
                                   float* y, int64_t y_stride, int B, int T, int F, int M, int hop,
                                   float* state, void* stream);

/* Initial state on every plan (additive in ABI 6).  A filter that starts from y[b][-1-j] = zi[b][j] is EXACTLY the zero-state
 * filter of an excitation whose first H = min(M, T) samples carry a correction, so golf_ltv_allpole_fwd_f32 / _bwd_f32 serve an
 * initial state on whichever plan they pick (time-chunked scan with its conditioning tiers, merged pass, serial, wave per
 * utterance) around these two memory-bound calls:
 *     c[t]  = sum_{i=t}^{M-1} A[t,i]*zi[i-t]            (t < H, else 0)
 *     xh[t] = ex[t]*G[t] - c[t]                          (0 <= t < T)
 *     y     = golf_ltv_allpole_fwd_f32(xh, gain == 1, a) ;   final state zf[j] = y[T-1-j] (j < T), zi[j-T] (j >= T)
 * The gain is applied here and never divided out of the head: it may hold an exact 0.
 *   ex (B, >=T) stride ex_stride   gain (B,F)   a (B,F,M)   zi (B,M)   xh (B,T) stride xh_stride, fully written
 *   1 <= T <= (F-1)*hop+1, 1 <= M <= 64.  One launch, no workspace.  A lane moves 4 consecutive samples with 16-byte accesses
 *   where the row address allows it (rows may be strided views with any start offset). */
int golf_ltv_allpole_head_fwd_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a, const float* zi,
                                  float* xh, int64_t xh_stride, int B, int T, int F, int M, int hop, void* stream);

/* Backward of the head (additive in ABI 6).  q (B, >=T) is what golf_ltv_allpole_bwd_f32 returned as g_ex for xh (gain == 1:
 * the reverse-time recursion g itself):
 *     g_ex[t]       = q[t]*G[t] (t < T), 0 (T <= t < Tx)         g_ex (B,Tx) stride g_ex_stride, fully written
 *     g_gain[f]     = up^T(q*ex)[f]                              (B,F)
 *     g_a_head[f,i] = up^T(-q[t]*zi[i-t])[f,i], t < H, i >= t    (B,F,M), zeros outside the head's frames; ADD it to the g_a
 *                                                                of golf_ltv_allpole_bwd_f32
 *     g_zi[j]       = -sum_{t < H, t+j < M} q[t]*A[t,t+j]        (B,M); the cotangent of zf[j+T] (j+T < M) is the caller's to add
 * Any of the four outputs may be NULL (not wanted); g_a_head or g_zi needs both a and zi.  At most two launches: g_ex
 * elementwise; then single-wave workgroups, one per (b,f) that GATHERS g_gain over the < 2 hop samples with a weight for the
 * frame, and one per utterance for g_a_head and g_zi.  Fixed summation order, no atomics: bit-reproducible. */
int golf_ltv_allpole_head_bwd_f32(const float* q, int64_t q_stride, const float* ex, int64_t ex_stride, const float* gain,
                                  const float* a, const float* zi, float* g_ex, int64_t g_ex_stride, int Tx, float* g_gain,
                                  float* g_a_head, float* g_zi, int B, int T, int F, int M, int hop, void* stream);

/* Conditioning and health status of the forward that last used `ws` (ABI 3).  The reference's sequential fp32
 * recursion degrades gracefully when an interpolated filter comes close to instability (models/filters.py:99-113 ->
 * torchlpc.sample_wise_lpc); the time-chunked algorithm keeps that behaviour by recomputing the
 * transition matrices of such chunks from fp64 trajectories and, for the worst utterances, scanning their boundary
 * states in fp64 (csrc/lpc_ss.hip, "conditioning tiers").  This call reports how often that happened and whether the
 * output is finite -- asynchronously, on `stream`, into 4 caller-owned DEVICE words the host reads when it likes:
 *   out[0]  utterances with at least one chunk whose matrix was recomputed from fp64 trajectories
 *   out[1]  utterances whose boundary states came from the fp64 scan (tier 3)
 *   out[2]  bit 0: a non-finite sample was written to y (an unstable filter is surfaced, not hidden);
 *           bit 1: a wait inside the pre-pass launch for the recomputed matrices ran into its bound (never observed; the
 *           result is then the fp32 matrices' -- less accurate, not undefined);
 *           bit 2: golf_ltv_allpole_bwd_f32 ran on this workspace with another boundary scan than the forward that filled
 *           it (GOLF_SS_FLAT_SCAN / _CHUNKED bits that differ between the two calls): its gradients are void.  Call this
 *           function after the backward to see it.
 *   out[3]  the largest |entry| over all transition matrices of the batch, as the bits of an fp32
 * (B,T,F,M,hop,flags) as given to the forward.  The serial and the wave-per-utterance algorithms form no matrices: all four
 * words 0. */
int golf_ltv_allpole_status_u32(const void* ws, size_t ws_bytes, int B, int T, int F, int M, int hop, int flags,
                                uint32_t* out, void* stream);

/* Custom backward of the above (what torchlpc's autograd.Function + autograd through
 * F.interpolate compute in the reference; closed form in SURVEY.md App. A-2):
 *     g[t]      = gy[t] - sum_i A[t+1+i,i]*g[t+1+i]      (reverse-time recursion)
 *     g_ex[t]   = g[t]*G[t]
 *     g_gain[f] = up^T(g*ex)[f]         g_a[f,i] = up^T(-g[t]*y[t-1-i])[f,i]
 *   gy,y (B,T) with strides; ws = the forward's workspace (same B,T,F,M,hop); flags = the forward's
 *   GOLF_SS_SERIAL / GOLF_SS_CHUNKED bits (ABI 2);
 *   g_ex (B,T) stride g_ex_stride, g_gain (B,F), g_a (B,F,M) are fully overwritten.
 *   Shapes without a ring (see above): the reverse-time recursion runs in the transposed form, lam_k = fma(-A[t,k], g[t],
 *   lam_{k+1}), one wave per utterance, into ws; one workgroup per (utterance, frame) then forms g_ex and the hat-weighted
 *   correlations in a fixed order -- no atomics, the gradients are bit-reproducible.  GOLF_EWORKSPACE when ws is smaller than
 *   golf_ltv_allpole_workspace_bytes_ex(B,T,F,M,hop,flags); M > 64 stays GOLF_EUNSUPPORTED. */
int golf_ltv_allpole_bwd_f32(const float* gy, int64_t gy_stride, const float* y, int64_t y_stride,
                             const float* ex, int64_t ex_stride, const float* gain, const float* a,
                             float* g_ex, int64_t g_ex_stride, float* g_gain, float* g_a,
                             int B, int T, int F, int M, int hop,
                             void* ws, size_t ws_bytes, int flags, void* stream);

/* a-1 in FLOAT64 (additive in ABI 6; csrc/lpc_any.hip, its double instantiations).  The same filter, the same up() interpolation and the same
 * T <= (F-1)*hop+1 rule as golf_ltv_allpole_fwd_f32 / _bwd_f32 -- models/filters.py:99-113, where torchlpc.sample_wise_lpc
 * (models/filters.py:112) is dtype-generic and is run, gradcheck'ed and rendered in double -- with everything on the recursion's
 * dependent chain in double: accumulators, interpolated coefficients, up(gain), the fed-back output.  For the utterances at the
 * edge of stability on which no fp32 recursion reaches 1e-4 (the status words above), for parity checks and for ground truth.
 *   io = 1  ex, gain, a, gy, y, g_ex, g_gain, g_a are DOUBLE buffers
 *   io = 0  they are fp32 buffers: widened at the load (exact), rounded once at the store; the arithmetic is the same
 *   state, zi, g_zi (B, M) and the workspace are doubles for either io (a chain of fp32 blocks continues from the unrounded
 *   outputs, and so stays on the bits of the one-shot call).
 * One wave per utterance, one lane per tap (the wave-per-utterance kernels of csrc/lpc_any.hip, for every shape: any
 * 1 <= M <= 64, hop >= 1, F >= 1, on or off the ring grid); the cost is that of one serial recursion per utterance.  Strides are
 * in elements of the io type, rows 64-bit addressed.  GOLF_EINVAL: a null required pointer, a non-positive size, T beyond
 * (F-1)*hop+1, a row stride below its width, io outside {0, 1}, a workspace that is missing, misaligned or too small;
 * GOLF_EUNSUPPORTED: M > 64 (or B*F >= 2^31 in the backward). */
/* The workspace of the backward below (autograd through models/filters.py:99-113): g (B, T) doubles, 256-byte aligned size;
 * 0 for a non-positive size.  The forward needs none. */
size_t golf_ltv_allpole_f64_workspace_bytes(int B, int T);
/* Forward, models/filters.py:99-113.  state == NULL: y[<0] = 0.  Else state (B, M) doubles, in and out, as in
 * golf_ltv_allpole_fwd_state_f32: y[b][-1-i] = state[b][i] on entry (replayed through the update by a prologue, so the
 * accumulators are rebuilt with the one-shot's operation sequence), state[b][i] = y[b][T-1-i] on return (for T < M the old
 * state shifted in behind them).  A sample's bits depend neither on where a block starts nor on the 64-sample I/O blocks:
 * blocks that start on frame boundaries, chained through `state` from zeros, give the bits of the one-shot call. */
int golf_ltv_allpole_fwd_f64(const void* ex, int64_t ex_stride, const void* gain, const void* a, void* y, int64_t y_stride,
                             int B, int T, int F, int M, int hop, double* state, int io, void* stream);
/* Backward of the above (models/filters.py:99-113 under autograd; the closed form of golf_ltv_allpole_bwd_f32), y the
 * forward's output and zi (nullable) the state it started from:
 *     g[t]      = gy[t] - sum_i A[t+1+i,i]*g[t+1+i]          into ws, (B, T) doubles
 *     g_ex[t]   = g[t]*G[t] (t < T), 0 (T <= t < g_ex_width)  (B, g_ex_width) stride g_ex_stride, fully written
 *     g_gain[f] = up^T(g*ex)[f]      g_a[f,i] = up^T(-g[t]*y[t-1-i])[f,i],  y[-1-j] = zi[j]
 *     g_zi[j]   = -sum_{t < min(T, M-j)} A[t,t+j]*g[t]       (the cotangent of a final state is the caller's to add)
 * Each of g_ex, g_gain, g_a, g_zi may be NULL: that gradient is not stored.  Two launches (the reverse recursion, one wave per
 * utterance; then one workgroup per (utterance, frame)), fixed summation order, no atomics: bit-reproducible. */
int golf_ltv_allpole_bwd_f64(const void* gy, int64_t gy_stride, const void* y, int64_t y_stride, const void* ex,
                             int64_t ex_stride, const void* gain, const void* a, const double* zi, void* g_ex,
                             int64_t g_ex_stride, int64_t g_ex_width, void* g_gain, void* g_a, double* g_zi, int B, int T,
                             int F, int M, int hop, void* ws, size_t ws_bytes, int io, void* stream);

/* a-5: inverse (analysis) filter e[t] = y[t] + sum_i A[t,i]*y[t-1-i].
 * Replaces LTVMinimumPhaseFilter.reverse -> fir_filt, models/filters.py:186-195, utils.py:433-441. */
int golf_ltv_inverse_f32(const float* y, int64_t y_stride, const float* a, float* e, int64_t e_stride,
                         int B, int T, int F, int M, int hop, void* stream);
/* Its backward (autograd through fir_filt's unfold + matmul in the reference; used when a decoder is trained with
 * `inverse_target`, ltng/vocoder.py:192-200):  g_y[t] = g_e[t] + sum_i A[t+1+i,i] g_e[t+1+i],
 * g_a[f,i] = up^T(g_e[t] * y[t-1-i]).  Either output may be NULL. */
int golf_ltv_inverse_bwd_f32(const float* g_e, int64_t g_e_stride, const float* y, int64_t y_stride, const float* a,
                             float* g_y, int64_t g_y_stride, float* g_a, int B, int T, int F, int M, int hop,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * LPC analysis (additive in ABI 6): audio -> (gain, a, rc) per frame by the autocorrelation method -- the estimate of
 * the time-varying predictor that a-1, a-4 and a-5 take as an input.  The reference has no such module; the definition is
 * the textbook one (oracle/make_lpc_tracks.py), with frame f of row b starting at sample origin + f*hop (origin =
 * -floor(W/2): the filters' centred frames; origin = 0: frames from sample 0) and x = 0 outside [0, T):
 *     s[k] = x[origin + f*hop + k] * window[k],   r[j] = sum_{n < W-j} s[n] s[n+j]  (j = 0..M),
 *     r[0] <- r[0] * (1 + eps_rel) + eps_abs     (silent frames stay well posed: a = 0),
 *     Levinson-Durbin from E_0 = r[0]:  k_i = -(r[i] + sum_{j<i} a_j r[i-j]) / E_{i-1},  a_j <- a_j + k_i a_{i-j},  a_i = k_i,
 *                                       E_i = E_{i-1} (1 - k_i^2),
 *     a (B, F, M) of A(z) = 1 + sum_i a_i z^-i (the sign of a-1, a-4, a-5),  rc (B, F, M) = k_1..k_M (golf_rc2lpc of it is a),
 *     gain (B, F) = sqrt(max(E_M, 0) / sum_k window[k]^2).
 * The frame is staged in fp32; lags, recursion and the whole backward are fp64 (reflection coefficients of speech reach
 * 0.998: fp32 lags or an fp32 recursion are 1e-3 .. 1e-1 off in a).  The forward keeps the regularised lags (B, F, M+1) as
 * doubles in `ws` (golf_lpc_analysis_workspace_bytes); the backward reads them from there (`lags`) and needs a second
 * buffer of the same size as its own `ws`.  g_gain, g_a, g_rc may each be NULL (an output nobody differentiates); rc may
 * be NULL in the forward.  g_x (B, T) is written in full, by a gather in a fixed order: no atomics, bit-reproducible.  The
 * window is a constant.  No call allocates or synchronises.
 * Refused before any launch: null required pointers (GOLF_EINVAL); M < 1, M > 64, W <= M, W > 4096 (a frame must fit
 * LDS), hop < 1, B*F >= 2^31 (GOLF_EUNSUPPORTED).
 * ------------------------------------------------------------------------------------------- */
size_t golf_lpc_analysis_workspace_bytes(int B, int F, int M);
int golf_lpc_analysis_fwd_f32(const float* x, int64_t x_stride, const float* window, float* gain, float* a, float* rc,
                              void* ws, size_t ws_bytes, int B, int T, int F, int M, int hop, int W, int64_t origin,
                              double eps_rel, double eps_abs, void* stream);
int golf_lpc_analysis_bwd_f32(const float* g_gain, const float* g_a, const float* g_rc, const float* x, int64_t x_stride,
                              const float* window, const void* lags, float* g_x, int64_t g_x_stride, void* ws,
                              size_t ws_bytes, int B, int T, int F, int M, int hop, int W, int64_t origin, double eps_rel,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Source-compensated LPC analysis (additive in ABI 6; csrc/lpc_analysis.hip): audio -> (gain, a, rc, source) per frame, with
 * the spectral tilt of the glottal source estimated beside the vocal tract and kept out of `a` -- iterative adaptive inverse
 * filtering (Alku, Speech Communication 11, 1992) without its integrators (the decoders' wavetable holds the flow derivative,
 * so lip radiation sits in the source), restated on the lags of the windowed frame.  The plain analysis above fits one
 * all-pole model to the whole spectrum and so absorbs the source's tilt; the GOLF decoders expect `a` to be the tract alone.
 * The float64 restatement in tests/sflpc_ref.py is the checker.  Frames, s[k], origin, x = 0 outside [0, T) and the window
 * are those of golf_lpc_analysis_fwd_f32.  With M the tract's order, Q >= 1 the source's, I = iterations >= 0, J = M + Q:
 *  1. r[j] = sum_{n < W-j} s[n] s[n+j]  (j = 0..J) in fp64, s one fp32 product;  r[0] <- r[0] (1 + eps_rel) + eps_abs, the
 *     only regularisation.
 *  2. Lags of the frame filtered by a polynomial c of order P, c_0 = 1:  rho_c[d] = sum_{p=0}^{P-d} c_p c_{p+d}  and
 *         (r o c)[j] = rho_c[0] r[j] + sum_{d=1}^{P} rho_c[d] (r[|j-d|] + r[j+d]),   ascending d, fp64;
 *     with eps = 0 it is the autocorrelation of the full convolution s * c.  It reads r up to j + P <= J.
 *  3. lev_n(.) is the Levinson-Durbin recursion of golf_lpc_analysis_fwd_f32 to order n.
 *  4. The first source polynomial, of order 1:  g = lev_1(r), that is g_1 = -r[1] / r[0]  (adaptive != 0), or
 *     g_1 = -preemphasis  (adaptive == 0).
 *  5. I times:  vt = lev_M((r o g)[0..M]);  g = lev_Q((r o vt)[0..Q]).
 *  6. (a, rc, .) = lev_M((r o g)[0..M]).
 *  7. gain = sqrt(max((r o a)[0], 0) / sum_k window[k]^2): the level of the audio through the tract's inverse alone, so
 *     that golf_ltv_residual_f32(x, gain, a) has unit local power like the table's pulses.
 * Outputs: gain (B, F); a (B, F, M); rc (B, F, M), the last stage's reflection coefficients (golf_rc2lpc of it is a), may be
 * NULL; source (B, F, Q) = g_1..g_Q, zero padded when I = 0, may be NULL.  With adaptive == 0, preemphasis == 0 and I = 0,
 * a and rc have the bits of golf_lpc_analysis_fwd_f32 and gain is its gain up to the rounding of (r o a)[0] against E_M.
 * A silent frame gives a = 0; every lag set is positive definite, so |rc| < 1; a NaN sample reaches only the frames that read
 * it.  One launch, one wave per frame, the frame staged in fp32 and everything after it fp64 in a fixed order: no workspace,
 * no atomics, bit-reproducible, a frame's bits depend on its samples only.  No call allocates or synchronises;
 * graph-capturable.  There is no gradient.
 * Refused before any launch: null x (with T > 0), window, gain or a; B < 0, T < 0, F < 1; x_stride < T; adaptive == 0 with
 * preemphasis not finite or |preemphasis| >= 1 (GOLF_EINVAL); M outside 1..64, Q outside 1..16, iterations outside 0..8,
 * W <= M + Q, W > 4096 (a frame must fit LDS), hop < 1, B*F >= 2^31 (GOLF_EUNSUPPORTED).  B == 0 returns GOLF_OK.
 * ------------------------------------------------------------------------------------------- */
int golf_lpc_source_filter_f32(const float* x, int64_t x_stride, const float* window, float* gain, float* a, float* rc,
                               float* source, int B, int T, int F, int M, int Q, int iterations, int adaptive,
                               double preemphasis, int hop, int W, int64_t origin, double eps_rel, double eps_abs,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * f0 analysis (additive in ABI 6): audio -> (f0, period, aperiodicity) per frame by YIN (de Cheveigne & Kawahara, JASA
 * 2002, steps 1-5) -- the f0 track that every decoder takes as an input, on the frame grid of the LPC analysis above.  The
 * reference gets f0 from a third-party CPU package (pyworld.dio, models/utils.py:596-602); this is not that estimator and
 * its tracks differ from the reference's f0 files.  The float64 restatement in tests/f0_ref.py is the checker.
 * Inputs: x (B, T) fp32 with unit inner stride and row stride x_stride; sample_rate; hop; W (integration window); tau_min,
 * tau_max (lag range in samples); threshold; rms_floor; origin; F.  Frame f of row b, with S = W + tau_max:
 *     s[k] = x[b, origin + f*hop + k]  for k in [0, S),  x = 0 outside [0, T);
 *  1. difference function   d[tau] = sum_{j<W} (s[j] - s[j+tau])^2                       tau = 0..tau_max
 *  2. cumulative-mean normalisation   d'[0] = 1,  d'[tau] = d[tau] tau / sum_{k=1..tau} d[k],  and d'[tau] = 1 where that
 *     running sum is 0 (a silent frame)
 *  3. search over [tau_min, tau_max]: the smallest tau with d'[tau] < threshold, then forward while tau+1 <= tau_max and
 *     d'[tau+1] < d'[tau]: that is tau* and found = true.  If no lag is below the threshold: tau* = argmin d' over the
 *     range, the smallest tau on ties, and found = false.
 *  4. parabolic refinement on d': with (a, b, c) = d'[tau*-1], d'[tau*], d'[tau*+1]: if tau*-1 >= 1, tau*+1 <= tau_max and
 *     a - 2b + c > 0 then delta = clamp((a - c) / (2 (a - 2b + c)), -1, 1), else delta = 0;
 *     period = tau* + delta;  ap = b - (a - c) delta / 4  (ap = b when delta = 0)
 *  5. voiced = found and mean_{j<W} s[j]^2 > rms_floor^2;  f0 = sample_rate / period if voiced, else 0 (the reference's
 *     convention: f0 == 0 is unvoiced, ltng/ae.py:98-101).
 * Outputs f0, period, ap, each (B, F) fp32 and each may be NULL (not written) as long as one is given; written in full by
 * one launch, no atomics, every sum in a fixed order: bit-reproducible, and a row's result does not depend on the batch it
 * sits in.  d is summed in fp32 (four partial sums per lag), the running sum of step 2 and steps 4-5 in fp64 from the fp32
 * d'.  Every loop is bounded by tau_max whatever the data.  No call allocates or synchronises; graph-capturable.
 * Refused before any launch: x NULL with T > 0, all three outputs NULL, B < 1, T < 0, F < 1, x_stride < T, sample_rate <= 0
 * (GOLF_EINVAL); hop < 1, tau_min < 1, tau_max <= tau_min, W < 1, S = W + tau_max > 16384 samples (a frame, its d' and the
 * partial sums must fit the 160 KiB of LDS: at most 132 KiB at S = 16384), B*F >= 2^31 (GOLF_EUNSUPPORTED).
 * ------------------------------------------------------------------------------------------- */
int golf_f0_yin_f32(const float* x, int64_t x_stride, float* f0, float* period, float* ap, int B, int T, int F, int hop,
                    int W, int tau_min, int tau_max, int64_t origin, double sample_rate, double threshold, double rms_floor,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * f0 tracking (additive in ABI 6): per-frame candidate periods and a minimum-cost path through them over the utterance, in
 * the manner of Praat's path finder (Boersma 1993), so that a frame is no longer decided on its own.  Two calls; the float64
 * restatement in tests/f0_track_ref.py is the checker of both.
 *
 * golf_f0_candidates_f32: the frames, d and the fp32-rounded d' of golf_f0_yin_f32 above (its steps 1-2 with the same
 * summation order, origin and F: one device function serves both), then instead of its search:
 *  3c. local minima: tau in [tau_min, tau_max] with d'[tau] < d'[tau-1] and (tau == tau_max or d'[tau] <= d'[tau+1]).  A NaN
 *      makes both comparisons false: a frame of NaN has none, and neither has a frame of zeros (d' = 1 everywhere).
 *  4c. of these the K with the smallest d'[tau] are kept, the smaller tau first among equal values; the n <= K kept ones
 *      are listed by ascending tau in slots 0 .. n-1, each refined as in step 4 above (period = tau + delta, ap).
 *  5c. slots n .. K-1 are absent: period = 0, ap = +inf.  A frame with mean_{j<W} s[j]^2 <= rms_floor^2 has n = 0.
 * Outputs cand_period, cand_ap, each (B, F, K) fp32 contiguous, every slot written by one launch; no atomics, fixed order,
 * bit-reproducible, a row does not depend on its batch; every loop is bounded by K (tau_max / 64 + 1) whatever the data;
 * no allocation or synchronisation, graph-capturable.  Refused before any launch: as golf_f0_yin_f32 (x NULL with T > 0 or
 * an output NULL, B < 1, T < 0, F < 1, x_stride < T: GOLF_EINVAL; hop < 1, tau_min < 1, tau_max <= tau_min, W < 1,
 * W + tau_max > 16384, B*F >= 2^31: GOLF_EUNSUPPORTED) and K outside 1..7 (GOLF_EUNSUPPORTED).
 *
 * golf_f0_viterbi_f32: cand_period, cand_ap (B, F, K) fp32 contiguous -> the path.  States: 0 is unvoiced, k+1 is slot k; a
 * slot is present iff period > 0 and ap is neither NaN nor +inf (periods are expected finite).  In float64, with u =
 * unvoiced_cost, lambda = lag_cost, gamma = jump_cost, sigma = switch_cost and p the period:
 *     local cost       l[f,0] = u;   l[f,k+1] = max(ap, 0) + lambda (log2 p - log2 lag_ref)   for a present slot
 *     transition cost  t(0,0) = 0;   t(0,j) = t(i,0) = sigma;   t(i,j) = gamma |log2 p[f,j] - log2 p[f-1,i]|   (i, j > 0)
 *     C[0,s] = l[0,s];   C[f,j] = l[f,j] + min_i (C[f-1,i] + t(i,j))   over the present i, the smaller i on a tie
 *     end state argmin_s C[F-1,s], the smaller s on a tie; then the backpointers are followed to frame 0.
 * Absent states are never entered and never predecessors, and no difference of infinities is formed; state 0 always
 * exists, so a path always exists.  Outputs: f0 (B, F) fp32, sample_rate / period of the chosen slot or 0 in state 0, and
 * state (B, F) int32; either may be NULL (not written), not both.  One launch, one wave per row, no atomics, one fixed
 * order: bit-reproducible and independent of the batch; no allocation or synchronisation, graph-capturable.  F is limited
 * only by B*F < 2^31: up to 4096 frames the backpointers live in LDS; beyond that the call needs a workspace of
 * golf_f0_viterbi_workspace_bytes(B, F, K) = 8 B F bytes (0 for F <= 4096, and 0 for sizes the call refuses), 8-byte
 * aligned, whose contents need not survive the call.  Refused before any launch: cand_period or cand_ap NULL, both outputs
 * NULL, B < 1, F < 1, sample_rate <= 0, lag_ref <= 0, a workspace that is needed and NULL or too small (GOLF_EINVAL); K
 * outside 1..7, B*F >= 2^31 (GOLF_EUNSUPPORTED).
 * ------------------------------------------------------------------------------------------- */
int golf_f0_candidates_f32(const float* x, int64_t x_stride, float* cand_period, float* cand_ap, int B, int T, int F, int hop,
                           int W, int tau_min, int tau_max, int K, int64_t origin, double rms_floor, void* stream);
size_t golf_f0_viterbi_workspace_bytes(int B, int F, int K);
int golf_f0_viterbi_f32(const float* cand_period, const float* cand_ap, float* f0, int* state, void* ws, size_t ws_bytes,
                        int B, int F, int K, double sample_rate, double lag_ref, double unvoiced_cost, double lag_cost,
                        double jump_cost, double switch_cost, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Streaming f0 tracking (additive in ABI 6): the path search of golf_f0_viterbi_f32 with its costs carried from call to call
 * and every frame decided a fixed number of frames late, so that a live analysis can feed a decoder stream.  The float64
 * restatement in tests/f0_stream_ref.py is the checker.
 * A call consumes frames [f_done, f_done + nf) of every row: cand_period, cand_ap (B, nf, K) fp32 contiguous.  States,
 * presence, l, t, C[f,j] and both tie rules are those of golf_f0_viterbi_f32 above, in float64 and summed in the same order:
 * C after frame f has the one-shot call's bits however the frames were cut into calls.  With e(f) = argmin_s C[f,s] (the
 * smaller s on a tie) and bp[f][j] the predecessor chosen for state j of frame f, the path to frame g seen from h >= g is
 *     s(g | h) = bp[g+1][ bp[g+2][ ... bp[h][ e(h) ] ... ] ],        s(g | g) = e(g).
 * With lag = L, frame g is decided once frame g + L has been consumed, as s(g | g + L); a call with flush != 0 ends the
 * utterance at F = f_done + nf and decides the frames still open as s(g | F - 1).  The result is a function of the candidates
 * and L alone; for L >= F - 1 it is the path of golf_f0_viterbi_f32.  With
 *     decided(n, flush) = n if flush, else max(n - L, 0);      n_out = decided(f_done + nf, flush) - decided(f_done, 0)
 * the call writes frames [decided(f_done, 0), decided(f_done + nf, flush)) to columns 0 .. n_out-1 of f0 and state, each
 * (B, n_out) with unit inner stride and row stride out_stride (elements): f0 fp32, sample_rate / period of the chosen slot or
 * 0 in state 0, and state int32; either may be NULL (not written), not both while n_out > 0.  Nothing else is written.
 * carry: golf_f0_viterbi_stream_state_bytes(B, K, lag) = B (192 + 40 lag) bytes, 8-byte aligned, one opaque block per row
 * (C, the logs and presence flags of the last frame, and the backpointers and candidate periods of the last `lag` frames,
 * because f0 of a late-decided frame comes from a call that has returned).  f_done == 0 starts an utterance and reads none
 * of it, so nobody has to clear it; a call reads and writes only its own rows' blocks and nothing beyond that size.  nf == 0
 * with flush and f_done > 0 is valid: it decides the last min(L, f_done) frames.
 * One launch, one wave per row, no atomics, one fixed order: bit-reproducible and independent of the batch; every loop is
 * bounded by nf, lag and K whatever the data holds; no allocation or synchronisation.  f_done is a launch argument.
 * Refused before any launch: B < 1, nf < 0, f_done < 0, cand_period or cand_ap NULL with nf > 0, nf == 0 without flush,
 * nf == 0 with f_done == 0, sample_rate <= 0, lag_ref <= 0, carry NULL, misaligned or smaller than the size above, both
 * outputs NULL while n_out > 0, out_stride < n_out (GOLF_EINVAL); K outside 1..7, lag outside 0..1024 (1024 frames are 10 s
 * at the recipe's hop), f_done + nf >= 2^31, B*nf >= 2^31 (GOLF_EUNSUPPORTED).  The size function answers 0 for B < 1 and
 * for the K and lag the call refuses.
 * ------------------------------------------------------------------------------------------- */
size_t golf_f0_viterbi_stream_state_bytes(int B, int K, int lag);
int golf_f0_viterbi_stream_f32(const float* cand_period, const float* cand_ap, float* f0, int* state, int64_t out_stride,
                               void* carry, size_t carry_bytes, int B, int nf, int K, int lag, int64_t f_done, int flush,
                               double sample_rate, double lag_ref, double unvoiced_cost, double lag_cost, double jump_cost,
                               double switch_cost, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Harmonic-plus-noise analysis (additive in ABI 6): (audio, f0) -> the controls of the harmonic-plus-noise decoders, per
 * frame on the grid of the analyses above (frame f is centred on sample f*hop): the amplitudes (and sine phases) that the
 * harmonic oscillator bank below takes and the log magnitudes that the zero-phase noise filter takes.  It is the classical
 * sinusoidal / harmonic-plus-noise analysis with a pitch-adaptive window and a per-frame chirp; the reference has no such
 * code.  The float64 restatement in tests/hna_ref.py is the checker.
 * Inputs: x (B, T) fp32, unit inner stride, row stride x_stride, 0 outside [0, T); f0 (B, F) fp32 in Hz, row stride
 * f0_stride, f0 <= 0 (or NaN) = unvoiced; K harmonics; n_mag noise bins (0: no noise output).  Every frame constant is
 * formed in fp64 from the fp32 inputs.  Frame f of row b:
 *  1. window length: voiced: n_per = max(periods, ceil(min_window f0 / sr)), L = min(max_window, floor(n_per sr / f0 + 0.5));
 *     unvoiced: L = unvoiced_window; L >= 2 in every case.
 *  2. offsets m = -floor(L/2) + i and window w[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / L), i = 0..L-1 (a Hann window on
 *     half-integer offsets: sum w = L/2, and the harmonics of a periodic signal are orthogonal over whole periods).
 *  3. phase of a voiced frame in cycles: omega = f0[f] / sr;  chirp s = (f0[f+1] - f0[f-1]) / (2 hop sr) if both neighbour
 *     frames exist and are voiced, the one-sided (f0[f+1] - f0[f]) / (hop sr) or (f0[f] - f0[f-1]) / (hop sr) if only
 *     one is, else 0;  phi(m) = omega m + s m^2 / 2.
 *  4. harmonics k = 1..K:  c_k = (2 / sum w) sum_i w[i] x[f hop + m] exp(-2 pi j k phi(m)),  c_k = 0 where k omega >= 0.5
 *     (the oscillator mutes those);  amplitudes[b,f,k-1] = |c_k|;  phases[b,f,k-1] = frac(arg(c_k) / 2 pi + 1/4) cycles,
 *     1/4 where c_k = 0: the sine phase at the frame's centre, the model being sum_k amp_k sin(2 pi (k phi(m) + phase_k)).
 *     Unvoiced frame: amplitudes and phases are 0.
 *  5. residual r[i] = x[f hop + m] - sum_k Re(c_k exp(2 pi j k phi(m))), x itself in an unvoiced frame;
 *     S_b = |sum_i w[i] r[i] exp(-j pi b m / (n_mag - 1))|^2 / sum w^2, b = 0..n_mag-1: the bins of the zero-phase noise
 *     filter, whose response is exp(log_mag); white noise of variance v gives E S_b = v.
 *  6. S_b <- mean of S over b-smooth .. b+smooth, reflected at both ends;  log_mag[b,f,b] = 0.5 log(S_b + eps).
 * Outputs: amplitudes (B, F, K); phases (B, F, K), may be NULL; log_mag (B, F, n_mag), may be NULL (then, and with
 * n_mag == 0, steps 5-6 are skipped); all contiguous, written in full by one launch of one workgroup per frame, no workspace,
 * no atomics, every sum in fp32 in a fixed order: bit-reproducible, and a row's result does not depend on its batch.
 * k phi mod 1 is exact integer arithmetic on phi(m) mod 1 formed in fp64 and kept as a 32-bit fraction of a cycle.
 * No call allocates or synchronises; graph-capturable.  There is no gradient.
 * Refused before any launch, all GOLF_EINVAL: B < 1, T < 0, F < 1; x NULL with T > 0, f0 or amplitudes NULL; x_stride < T,
 * f0_stride < F; K outside 1..256; n_mag outside {0, 2..513}; hop < 1; periods < 2; max_window outside 2..2048 (a frame
 * must fit LDS); min_window outside 1..max_window; unvoiced_window outside 2..2048; smooth < 0 or smooth >= n_mag > 0;
 * sample_rate <= 0; eps < 0; B*F >= 2^31.
 * ------------------------------------------------------------------------------------------- */
int golf_harmonic_analysis_f32(const float* x, int64_t x_stride, const float* f0, int64_t f0_stride, float* amplitudes,
                               float* phases, float* log_mag, int B, int T, int F, int K, int n_mag, int hop, int periods,
                               int min_window, int max_window, int unvoiced_window, int smooth, double sample_rate,
                               double eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same analysis at a position of a longer utterance (additive in ABI 6): frames f_first .. f_first + n_frames - 1 from
 * windows of the inputs, for the block-by-block form (analysis_stream.HarmonicNoiseStream).  Frames, samples, steps 1-6, the
 * limits and the properties are those of golf_harmonic_analysis_f32: it is the same kernel and the same launch shape, and a
 * frame has the one-shot call's bits.  All positions are those of the utterance, int64 (a live stream may run for hours):
 *   x (B, n_x), row stride x_stride: samples [x_t0, x_t0 + n_x).  x_t0 >= 0: the buffer never holds the zeros before sample 0;
 *     a sample t < 0 reads as 0, and with last != 0 so does t >= x_t0 + n_x (the utterance ends there: T = x_t0 + n_x).
 *   f0 (B, n_f0), row stride f0_stride: frames [f0_first, f0_first + n_f0), f0_first >= 0.  In step 3 the neighbour f - 1
 *     exists iff f - 1 >= f0_first and the neighbour f + 1 iff f + 1 < f0_first + n_f0: the one-shot's f > 0 and f + 1 < F,
 *     given the preconditions below, with F = f0_first + n_f0 when last != 0.
 *   amplitudes (B, n_frames, K), phases (B, n_frames, K) or NULL, log_mag (B, n_frames, n_mag) or NULL: column j is frame
 *     f_first + j.
 * With Lmax = max(max_window, unvoiced_window), the longest window a frame can take, refused before any launch, all
 * GOLF_EINVAL, each naming its argument -- a mistake in the caller's bookkeeping is an error, never another chirp or a
 * window padded with zeros:
 *   B < 1, n_x < 0, n_f0 < 1, n_frames < 1; x NULL with n_x > 0, f0 or amplitudes NULL; x_stride < n_x, f0_stride < n_f0;
 *   the limits of golf_harmonic_analysis_f32 on K, n_mag, hop, periods, the windows, smooth, sample_rate and eps;
 *   B*n_frames >= 2^31; x_t0, f0_first or (f_first + n_frames) hop outside 0..2^62;
 *   x_t0 > max(0, f_first hop - floor(Lmax/2)): a frame could read below the buffer;
 *   f0_first > max(f_first - 1, 0) or f_first + n_frames > f0_first + n_f0: f0 does not cover the frames and the neighbour
 *     before the first;
 *   with last == 0: (f_first + n_frames - 1) hop + Lmax - floor(Lmax/2) > x_t0 + n_x (a window could reach beyond the buffer)
 *     or f_first + n_frames + 1 > f0_first + n_f0 (the last frame's next neighbour has not come).
 * ------------------------------------------------------------------------------------------- */
int golf_harmonic_analysis_stream_f32(const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* f0,
                                      int64_t f0_stride, int64_t f0_first, int n_f0, float* amplitudes, float* phases,
                                      float* log_mag, int B, int64_t f_first, int n_frames, int last, int K, int n_mag,
                                      int hop, int periods, int min_window, int max_window, int unvoiced_window, int smooth,
                                      double sample_rate, double eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spectral-envelope analysis (additive in ABI 6): (audio, f0) -> the control of the cepstral harmonic filter (LTVCepFilter:
 * ceps) and the response rows of the STFT-domain frame filter (exp(log_env)), per frame on the grid of the analyses above
 * (frame f is centred on sample f*hop).  It is a pitch-adaptive envelope estimator of the CheapTrick kind: an f0-sized
 * window, a power spectrum, smoothing over 2 f0 / 3 and cepstral liftering; the reference has no such code.  The float64
 * restatement in tests/env_ref.py is the checker.
 * Inputs: x (B, T) fp32, unit inner stride, row stride x_stride, 0 outside [0, T); f0 (B, F) fp32 in Hz, row stride
 * f0_stride, f0 <= 0 (or NaN) = unvoiced; n = n_fft, a power of two in [64, 2048], nb = n/2 + 1 bins; 0 <= n_ceps <= nb.
 * Every frame constant is formed in fp64 from the fp32 inputs.  Frame f of row b:
 *  1. effective f0: fe = min(max(f0, f0_floor), f0_ceil) if voiced, else unvoiced_f0.
 *  2. window: hw = floor(1.5 sr / fe + 0.5), offsets m = -hw..hw, w(m) = 0.5 + 0.5 cos(2 pi m fe / (3 sr)), a Hann window
 *     three periods wide;  xw(m) = w(m) x[f hop + m];  the DC the window sees is removed: xw <- xw - w (sum xw / sum w).
 *  3. power spectrum: P[k] = |sum_m xw(m) exp(-2 pi j k m / n)|^2 / sum w^2, k = 0..n/2; white noise of variance v gives
 *     E P = v, the unit of golf_harmonic_analysis_f32's S_b.
 *  4. DC correction: r0 = fe n / sr bins;  for each k < r0, with u = r0 - k, the linear interpolation of P (as step 3 left
 *     it) at the bin coordinate u, between floor(u) and min(floor(u) + 1, n/2), is added to P[k].
 *  5. smoothing over 2 fe / 3: P is extended evenly about bin 0 and about bin n/2 and read as piecewise constant on the
 *     cells [k - 1/2, k + 1/2);  Ps[k] is its mean over [k - r, k + r], r = r0 / 3, a cell partly inside counting by its
 *     covered fraction.
 *  6. L[k] = log(Ps[k] + eps);  c[q], q = 0..n/2, is the inverse real DFT of the even extension of L.
 *  7. lifter: c'[q] = c[q] sinc(fe q / sr) ((1 - 2 q1) + 2 q1 cos(2 pi fe q / sr)), sinc(t) = sin(pi t) / (pi t), 1 at q = 0.
 *  8. log_env[b,f,k] = 0.5 Re DFT(even extension of c')[k] + off, the natural log of the magnitude envelope;
 *     ceps[b,f,m] = 0.5 c'[m] + (m == 0) off, m < n_ceps, in LTVCepFilter's convention log|H|[k] = c_0 + 2 sum_{m>=1} c_m
 *     cos(2 pi k m / n): with n_ceps = nb its response is exp(log_env) up to rounding, a smaller n_ceps truncates further;
 *     off = voiced_offset on voiced frames, 0 on unvoiced ones.  (The estimate is in white-noise units, and a pulse train
 *     whose harmonics have the amplitude sqrt(2 f0 / sr) has half the power density of unit white noise: voiced_offset =
 *     0.5 ln 2 makes a voiced frame return log|H| of the filter the pulse train went through.)
 * Outputs: log_env (B, F, nb) and ceps (B, F, n_ceps), contiguous, either may be NULL, not both; written in full by one
 * launch of one workgroup per frame, no workspace, no atomics, every sum in fp32 in a fixed order: bit-reproducible, and a
 * row's result does not depend on its batch.  The three transforms are fp32 FFTs in LDS; step 5 sums each bin's cells
 * directly (no difference of running sums); eps is rounded to fp32.  No call allocates or synchronises; graph-capturable.
 * There is no gradient.  The window is at least three periods wide and must fit n, so r0 >= 3 and r >= 1 bin always.
 * Refused before any launch, GOLF_EINVAL, each naming its argument: B < 1, T < 0, F < 1; f0 NULL, x NULL with T > 0; both
 * outputs NULL, ceps with n_ceps == 0; x_stride < T, f0_stride < F; hop < 1; sample_rate <= 0; eps <= 0; n_ceps outside
 * 0..nb; f0_floor <= 0, f0_floor > f0_ceil, f0_ceil > sr/4; unvoiced_f0 outside [f0_floor, f0_ceil]; q1 or voiced_offset
 * NaN; floor(1.5 sr / f0_floor + 0.5) > n/2 - 1 (the longest window must fit the transform); B*F >= 2^31.  n_fft not a power
 * of two or outside [64, 2048]: GOLF_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int golf_spectral_envelope_f32(const float* x, int64_t x_stride, const float* f0, int64_t f0_stride, float* log_env,
                               float* ceps, int B, int T, int F, int n_fft, int n_ceps, int hop, double sample_rate,
                               double f0_floor, double f0_ceil, double unvoiced_f0, double q1, double eps,
                               double voiced_offset, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same analysis at a position of a longer utterance (additive in ABI 6): frames f_first .. f_first + n_frames - 1 from
 * windows of the inputs, for the block-by-block form (analysis_stream.SpectralEnvelopeStream).  Frames, steps 1-8, the limits
 * and the properties are those of golf_spectral_envelope_f32: it is the same kernel and the same launch shape, and a frame
 * has the one-shot call's bits.  All positions are those of the utterance, int64:
 *   x (B, n_x), row stride x_stride: samples [x_t0, x_t0 + n_x), x_t0 >= 0.  A sample t < 0 reads as 0, and with last != 0 so
 *     does t >= x_t0 + n_x (the utterance ends there: T = x_t0 + n_x).
 *   f0 (B, n_f0), row stride f0_stride: frames [f0_first, f0_first + n_f0).  A frame reads its own f0 only, no neighbour's.
 *   log_env (B, n_frames, nb), ceps (B, n_frames, n_ceps), either may be NULL, not both: column j is frame f_first + j.
 * A frame reads the samples f hop - hw .. f hop + hw, hw <= hwmax = floor(1.5 sr / f0_floor + 0.5), the half window of the
 * lowest f0.  Refused before any launch, all GOLF_EINVAL, each naming its argument -- a mistake in the caller's bookkeeping is
 * an error, never a window padded with zeros:
 *   B < 1, n_x < 0, n_f0 < 1, n_frames < 1; x NULL with n_x > 0, f0 NULL; both outputs NULL, ceps with n_ceps == 0;
 *   x_stride < n_x, f0_stride < n_f0; the limits of golf_spectral_envelope_f32 on n_fft (GOLF_EUNSUPPORTED), n_ceps, hop,
 *   sample_rate, eps, f0_floor, f0_ceil, unvoiced_f0, q1 and voiced_offset; B*n_frames >= 2^31;
 *   x_t0, f0_first or (f_first + n_frames) hop outside 0..2^62;
 *   x_t0 > max(0, f_first hop - hwmax): a frame could read below the buffer;
 *   f0_first > f_first or f_first + n_frames > f0_first + n_f0: f0 does not cover the frames;
 *   with last == 0: (f_first + n_frames - 1) hop + hwmax + 1 > x_t0 + n_x (a window could reach beyond the buffer).
 * ------------------------------------------------------------------------------------------- */
int golf_spectral_envelope_stream_f32(const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* f0,
                                      int64_t f0_stride, int64_t f0_first, int n_f0, float* log_env, float* ceps, int B,
                                      int64_t f_first, int n_frames, int last, int n_fft, int n_ceps, int hop,
                                      double sample_rate, double f0_floor, double f0_ceil, double unvoiced_f0, double q1,
                                      double eps, double voiced_offset, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The residual, fused (additive in ABI 6; csrc/lpc_residual.hip): (audio, gain, a) -> the decoder's excitation estimate, the
 * audio through the inverse of its all-pole filter divided by the interpolated gain, in one launch.  It is the input of the
 * glottal-source analysis below, and the definition its block-by-block form is exact against: every quantity of sample t is
 * a function of t and of the two frames around it, never of a running product.  The float64 restatement in
 * tests/residual_ref.py is the checker.
 * Inputs: x (B, T) fp32, unit inner stride, row stride x_stride; gain (B, F) and a (B, F, M) fp32, contiguous, as
 * golf_lpc_analysis_fwd_f32 writes them; 1 <= M <= 64, hop >= 1.  T' = min(T, (F - 1) hop + 1).  For t < T':
 *   f = min(floor(t / hop), F - 2), or 0 when F == 1;
 *   w = (float)(t - f hop) / (float)hop, one correctly rounded fp32 division of two exact integers;
 *   A[t,i] = fmaf(w, a[f+1,i] - a[f,i], a[f,i]), i < M  (a[f,i] itself when F == 1);
 *   G[t]   = fmaf(w, gain[f+1] - gain[f], gain[f])      (gain[f] itself when F == 1);
 *   num[t] = x[t] + sum_{i < M, t-1-i >= 0} A[t,i] x[t-1-i], accumulated in fp32 with fmaf in ascending i from x[t]: the
 *            bits of golf_ltv_inverse_f32;
 *   e[t]   = num[t] / G[t], one correctly rounded fp32 division (no reciprocal approximation).  A zero gain gives what
 *            IEEE 754 gives (inf or NaN); golf_lpc_analysis_fwd_f32 never returns 0.
 * Output: e (B, T'), row stride e_stride, written in full by one launch of one workgroup per (row, tile of 256 samples); the
 * tile's samples and the M before them are staged in LDS.  No workspace, no atomics, a fixed order: bit-reproducible, and a
 * row's result does not depend on its batch.  No call allocates or synchronises; graph-capturable.  There is no gradient
 * (golf_ltv_inverse_f32 has one).
 * Refused before any launch, GOLF_EINVAL, each naming its argument: B < 1, T < 1, F < 1; any pointer NULL; M outside 1..64;
 * hop < 1; x_stride < T, e_stride < T'; B * ceil(T' / 256) >= 2^31.
 * ------------------------------------------------------------------------------------------- */
int golf_ltv_residual_f32(const float* x, int64_t x_stride, const float* gain, const float* a, float* e, int64_t e_stride,
                          int B, int T, int F, int M, int hop, void* stream);

/* The same kernel at a position of a longer utterance (additive in ABI 6), for the block-by-block form
 * (analysis_stream.ResidualStream): samples t_first .. t_first + n_out - 1, each with the one-shot call's bits.  All
 * positions are those of the utterance, int64:
 *   x (B, n_x), row stride x_stride: samples [x_t0, x_t0 + n_x); a sample t < 0 reads as 0 (and is never a tap);
 *   gain (B, n_fr) and a (B, n_fr, M), contiguous: frames [fr_first, fr_first + n_fr);
 *   e (B, n_out), row stride e_stride: column j is sample t_first + j.
 * With last == 0 the utterance goes on: f = floor(t / hop) without a clamp, and frame f + 1 must be in the buffer.  With
 * last != 0 the utterance has F = fr_first + n_fr frames: the clamp f <= F - 2 applies (f = 0 when F == 1) and no sample
 * at or beyond (F - 1) hop + 1 exists.
 * Refused before any launch, all GOLF_EINVAL, each naming its argument -- a mistake in the caller's bookkeeping is an error,
 * never another interpolation:
 *   B < 1, n_x < 1, n_fr < 1, n_out < 1; any pointer NULL; M outside 1..64; hop < 1; x_stride < n_x, e_stride < n_out;
 *   x_t0, t_first or (fr_first + n_fr) hop outside 0..2^62; B * ceil(n_out / 256) >= 2^31;
 *   x_t0 > max(0, t_first - M): a tap could read below the buffer;
 *   x_t0 + n_x < t_first + n_out: x does not cover the samples;
 *   with last == 0: floor((t_first + n_out - 1) / hop) + 1 >= fr_first + n_fr (the next frame of the last sample has not come);
 *   with last != 0: t_first + n_out > (F - 1) hop + 1;
 *   fr_first > the frame f of sample t_first (as defined above, with the clamp when last != 0): its frame is missing. */
int golf_ltv_residual_stream_f32(const float* x, int64_t x_stride, int64_t x_t0, int n_x, const float* gain, const float* a,
                                 int64_t fr_first, int n_fr, float* e, int64_t e_stride, int B, int64_t t_first, int n_out,
                                 int last, int M, int hop, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Glottal-source analysis (additive in ABI 6): (the harmonics of a residual, f0) -> the control of the glottal-flow wavetable
 * (IndexedGlottalFlowTable: table_select_weight), per frame on the grid of the analyses above.  The residual is the audio
 * through golf_ltv_inverse_f32, divided by the gain; its harmonics are what golf_harmonic_analysis_f32 writes.  Each frame's
 * harmonics are matched against every table row at every one of n_phi phase shifts, and the best row and shift are refined;
 * the reference has no such code.  The float64 restatement in tests/glottal_ref.py is the checker.
 * Inputs: amplitudes, phases (B, F, H) fp32, contiguous, exactly as golf_harmonic_analysis_f32 writes them (sine phases in
 * cycles): c_h = amp_h exp(2 pi j (phase_h - 1/4)), h = 1..H;  f0 (B, F) fp32 in Hz, row stride f0_stride, f0 <= 0 (or NaN)
 * = unvoiced.  The plan of a table (K, L), built once per table (functional.glottal_plan), contiguous fp32:
 *   spectrum (K, H, 2): S[k,h] = 2 rfft(table[k])[h] / L (re, im), h = 1..H; entries with h > L/2 are zero;
 *   norms (K, H):     N[k,h] = sum_{i<=h} |S[k,i]|^2;
 *   cross (K-1, H):   X[k,h] = sum_{i<=h} Re(S[k,i] conj(S[k+1,i])), both summed in float64 over the fp32 S and rounded once.
 * Every frame constant is formed in fp64 from the fp32 inputs.  Frame f of row b:
 *  1. Hf = the number of h in 1..H with h (double)f0 / sr < 0.5, the harmonics golf_harmonic_analysis_f32 does not mute (the
 *     same expression: the two kernels agree on it bit for bit);  E2 = sum_{h<=Hf} amp_h^2.
 *  2. unvoiced, Hf = 0 or E2 = 0 (or NaN):  w = NaN, theta = 0, rho = 0, and nothing else is computed.
 *  3. C[k,j] = sum_{h<=Hf} Re(c_h conj(S[k,h]) exp(-2 pi j h j / n_phi)), k = 0..K-1, j = 0..n_phi-1; the argument h j mod
 *     n_phi is exact integer arithmetic.  rho[k,j] = C[k,j] / sqrt(N[k,Hf] E2); a row with N[k,Hf] = 0 scores 0.
 *  4. (k*, j*) = argmax rho, the smaller k, then the smaller j, on exact ties.
 *  5. phase: a parabola through rho[k*, j*-1], rho[k*, j*], rho[k*, j*+1], columns modulo n_phi;  d = its vertex, in
 *     [-1/2, 1/2], 0 when the curvature is 0;  theta = frac((j* + d) / n_phi), in [0, 1).
 *  6. row, at column j*, for each existing pair (k0, k0+1), k0 = k*-1 then k0 = k*: with c0 = C[k0,j*], c1 = C[k0+1,j*],
 *     n00 = N[k0,Hf], n11 = N[k0+1,Hf], n01 = X[k0,Hf], the blend (1-p) row_k0 + p row_{k0+1} scores
 *     ((1-p) c0 + p c1) / sqrt(((1-p)^2 n00 + 2 p (1-p) n01 + p^2 n11) E2) (0 when the bracket is not positive), largest at
 *     p = u / (u + v), u = c1 n00 - c0 n01, v = c0 n11 - c1 n01, clipped to [0, 1], p = 0 when u + v = 0.  The better pair
 *     is taken (the first on a tie), and (rho[k*,j*], k*) is kept unless a pair beats it strictly:
 *     w = (k0 + p) / (K - 1), rho = that score.
 * w is the inverse of the oscillator's row-pair interpolation (blend_tables), theta the oscillator's wrapped table phase at
 * the frame's centre, rho in [-1, 1] a voicing / fit confidence (the normalised correlation of the frame's harmonics with
 * the chosen pulse).
 * Outputs: w, theta, rho (B, F) each, contiguous; each may be NULL, not all three; written in full by one launch of one
 * workgroup per frame.  The K x n_phi scores never reach memory: a lane keeps 16 of them in registers and the argmax is
 * reduced inside the workgroup.  The search of steps 3-4 has fp32 operands (c_h and exp(.) rounded to fp32, D = c_h conj(S)
 * formed in fp32) and fp32 accumulation with fmaf in ascending h.  Neighbouring rows differ by 1e-4 .. 1e-3 in rho, so two
 * neighbouring cells can tie within fp32 rounding, and steps 5-6 are discontinuous in (k*, j*); so the 5 x 5 scores around the
 * fp32 winner are formed again in fp64 from the fp32 inputs (c_h unrounded), (k*, j*) is taken among the inner 3 x 3 by the
 * rule of step 4, and steps 5-6 run in fp64 on those scores.  A frame then differs from a float64 computation of the whole
 * definition by the rounding of its three outputs, unless two cells that are not neighbours tie within fp32 rounding.
 * No workspace, no atomics, every sum in a fixed order: bit-reproducible, and a row's result does not depend on its batch.
 * No call allocates or synchronises; graph-capturable.  There is no gradient.
 * Refused before any launch, GOLF_EINVAL, each naming its argument: B < 1, F < 1; H outside 1..256; K outside 2..1024; any
 * input or plan pointer NULL; all three outputs NULL; f0_stride < F; sample_rate <= 0; B*F >= 2^31.  n_phi not a power of
 * two or outside [8, 4096]: GOLF_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int golf_glottal_match_f32(const float* amplitudes, const float* phases, const float* f0, int64_t f0_stride,
                           const float* spectrum, const float* norms, const float* cross, float* w, float* theta, float* rho,
                           int B, int F, int H, int K, int n_phi, double sample_rate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a-4: frame-wise LTI all-pole + windowed overlap-add — GOLF-ff end filter.
 * Replaces LTVMinimumPhaseFilter.forward, models/filters.py:131-184 (pad, unfold, lpc_synthesis ->
 * torchaudio.functional.lfilter models/lpc.py:11-16, diagonal conv_transpose1d OLA, normalise).
 *   x = ex*up(gain) (length Tx = min(T_ex, (F-1)*hop+1)), zero-padded by W/2 each side;
 *   frame f = x_pad[f*hop .. f*hop+W), nfr = (Tx + 2*(W/2) - W)/hop + 1 <= F frames,
 *   filt_f = LTI all-pole a[b,f,:] from zero state;
 *   y[n] = sum_f window[k]*filt_f[k] / sum_f window[k],  n = f*hop - W/2 + k,  n in [0, Ty),
 *   Ty = (nfr-1)*hop + W - 2*(W/2).
 *   window (W) fp32; requires W >= 2*hop.  `centred==0` handling (drop hop/2, reflect pad) is done
 *   by the host wrapper.  ws: golf_lti_frames_workspace_bytes().
 *   Shapes: any order 1 <= M <= 64, any hop >= 1, any even W >= 2*hop (M > 64: GOLF_EUNSUPPORTED).  Where a ring width
 *   w in {8,16,24,32,40} has M <= w - 2 and w <= hop, the frames run on the ring kernels of lpc_ff.hip (the block
 *   recursion for M <= 22, W % 32 == 0, hop % 4 == 0; the quad kernel for W % w == 0; a lane per frame otherwise); every
 *   other shape (M in 39 .. 64, or hop below the ring width M needs) runs one wave per frame with one lane per tap
 *   (lpc_ff_any.hip).  The overlap-add is the same kernel for all of them. */
size_t golf_lti_frames_workspace_bytes(int B, int Tx, int F, int M, int hop, int W);

int golf_lti_frames_ola_fwd_f32(const float* ex, int64_t ex_stride, const float* gain, const float* a,
                                const float* window, float* y, int64_t y_stride,
                                int B, int Tx, int F, int M, int hop, int W, int Ty,
                                void* ws, size_t ws_bytes, void* stream);

/* Streaming form (additive in ABI 6): the same frames and overlap-add, block by block, in global sample / frame indices.
 * x[n] = ex[n]*up(gain)[n] for 0 <= n < x_end (0 elsewhere); frame f covers x[f*hop - W/2, f*hop - W/2 + W); y as above.
 * One call filters frames [f0, f0+nf) -- each frame once over the stream -- and writes samples [n0, n0+ny) to y (B, ny).
 *   ex      window of the excitation: global samples [x0, x0+nx), row stride ex_stride
 *   gain    rows [g0, g0+ng) (B, ng);  a  rows [a0, a0+na) (B, na, M), both contiguous
 *   x_end, g_end  -1 while the utterance is open; once it has ended, Tx = min(T_ex, (g_end-1)*hop+1) and F: the frame range
 *           and the normaliser are clipped to nfr = (Tx + 2*(W/2) - W)/hop + 1 and up(gain) to segment F-2 as in the one-shot
 *   carry   caller-owned (B, S, W) fp32 device buffer, zero-initialised, S = ceil(W/hop) - 1 (golf_lti_frames_stream_state_bytes):
 *           the last S filtered frames, frame f at slot f % S
 *   ws      scratch of 4*B*(S+nf)*W bytes, 256-aligned (NULL with nf = ny = 0)
 * Requirements (refused before any launch): W >= 2*hop, M <= 38; the windows cover frames [f0, f0+nf), their samples and
 * the gain rows those samples interpolate; the samples [n0, n0+ny) need no frame >= f0+nf (nor one older than the carry
 * holds); frame f0 reaches no sample before n0; after the call no unwritten sample needs a frame older than f0+nf-S (write
 * every sample the frames finish).  Each sample sums its frames in ascending f with fmaf, the window sum as its normaliser,
 * as the one-shot does.  The block recursion serves the shapes where the one-shot uses it, with the fp64 feedback tier chosen
 * per FRAME from its own kappa (the one-shot chooses per wave of 4 frames): a frame's bits depend on its own inputs only, so
 * the output does not depend on how the input is split into calls.  Other shapes run a direct-form kernel; any M <= 38 and
 * hop >= 1.  Two launches (frames, then overlap-add); none when nf = ny = 0.  No host<->device synchronisation. */
size_t golf_lti_frames_stream_state_bytes(int B, int W, int hop, int M);
int golf_lti_frames_ola_stream_f32(const float* ex, int64_t ex_stride, int64_t x0, int nx, int64_t x_end,
                                   const float* gain, int64_t g0, int ng, int64_t g_end, const float* a, int64_t a0, int na,
                                   const float* window, int64_t f0, int nf, float* y, int64_t y_stride, int64_t n0, int ny,
                                   int B, int M, int hop, int W, float* carry, void* ws, size_t ws_bytes, void* stream);

/* STFT-domain frame filter, streaming form (additive in ABI 6): the arithmetic of LTVCepFilter (NHV) and DiffWorldSPFilter
 * (WORLD) -- torch.stft(center=True, reflect) -> multiply by a per-frame response -> torch.istft -- frame by frame, in global
 * sample / frame indices.  With n = n_fft, w = window:
 *   frame f covers x[f*hop - n/2, f*hop + n/2); an index i < 0 reads x[-i]; once the utterance has ended an index i >= x_end
 *   reads x[2(x_end-1) - i];   u_f = Re IFFT(FFT(w * frame_f) * H_f);
 *   y[m] = sum_f w[k]*u_f[k] / sum_f w[k]^2,  k = m + n/2 - f*hop, over the frames 0 <= f < frames that cover m.
 * One call filters frames [f0, f0+nf) -- each frame once over the stream -- and writes samples [n0, n0+ny) to y (B, ny).
 *   x       window of the input: global samples [x0, x0+nx), row stride x_stride
 *   h       response rows [h0, h0+nh) on bins 0 .. n/2, contiguous: (B, nh, n/2+1) real (h_kind 0) or (B, nh, n/2+1, 2)
 *           interleaved complex (h_kind 1); bins above n/2 follow by Hermitian symmetry
 *   x_end, frames_end  -1 while the utterance is open; once it has ended, its length T > n/2 and frames = min(1 + T/hop, F)
 *           (at most 1 + T/hop): they switch on the right reflection and clip the frame range and the normaliser; the
 *           output then ends at hop*(frames-1)
 *   carry   caller-owned (B, S, n) fp32 device buffer, zero-initialised, S = ceil(n/hop) - 1
 *           (golf_stft_filter_stream_state_bytes): the last S filtered frames, frame f at slot f % S
 *   ws      scratch of 4*B*(S+nf)*n bytes, 256-aligned (NULL with nf = ny = 0)
 * Refused before any launch: null pointers; n not a power of two in [64, 2048] (GOLF_EUNSUPPORTED); n < 2*hop; windows that
 * do not cover frames [f0, f0+nf), the samples they read (reflections included: the last frame of an utterance whose length
 * is a multiple of hop reads x[T-1-n/2], one sample before its own span) or their response rows; samples [n0, n0+ny) that
 * need a frame >= f0+nf or one older than the carry holds; frame f0 reaching a sample before n0; leaving unwritten a sample
 * that needs a frame older than f0+nf-S; x_end <= n/2.
 * The transform is a radix-4 Stockham FFT in LDS with twiddles from sincospif; a frame's bits depend on its own samples and
 * its own response row only, and each sample sums its frames in ascending f with fmaf, the normaliser in the same order, so
 * the output does not depend on how the input is split into calls.  Two launches (frames, then overlap-add); none when
 * nf = ny = 0.  No host<->device synchronisation. */
size_t golf_stft_filter_stream_state_bytes(int B, int n_fft, int hop);
int golf_stft_filter_frames_stream_f32(const float* x, int64_t x_stride, int64_t x0, int nx, int64_t x_end, const float* h,
                                       int64_t h0, int nh, int h_kind, int64_t frames_end, const float* window, int64_t f0,
                                       int nf, float* y, int64_t y_stride, int64_t n0, int ny, int B, int n_fft, int hop,
                                       float* carry, void* ws, size_t ws_bytes, void* stream);

/* Backward of the STFT-domain frame filter over a whole utterance (additive in ABI 6): the forward above called once with
 * x0 = h0 = f0 = n0 = 0, x_end = T, frames_end = frames = min(1 + T/hop, F), ny = Ty = hop*(frames-1) and a zero carry --
 * what autograd computes in the reference through torch.stft, the product and torch.istft (closed form restated in float64 in
 * tests/stft_filter_ref.py).  With q = gy / norm, pad = n/2, v_f the windowed frame of the forward and V_f = FFT(v_f), recomputed:
 *   gu_f[k] = w[k]*q[f*hop - pad + k] (0 outside [0, Ty));   GU_f = FFT(gu_f);
 *   g_h[b,f,kk] = c[kk]*conj(V_f[kk])*GU_f[kk]/n on bins 0 .. n/2, c = 1 at bins 0 and n/2 and 2 elsewhere: (re, im) for
 *           h_kind 1, the real part for h_kind 0; rows frames <= f < F are zeros;
 *   gv_f = Re IFFT(conj(Hext_f)*GU_f);   G[p] = sum_f w[k]*gv_f[k], k = p + pad - f*hop, frames in ascending f with fmaf;
 *   g_x[r] = G[r] + G[-r] (1 <= r <= pad) + G[2(T-1) - r] (where that position is >= T): a gather, no atomics.
 *   gy (B, Ty), x (B, T), g_x (B, T) with row strides; h and g_h contiguous as in the forward, F rows each.
 *   g_x or g_h may be NULL (not both): the inverse transforms and the gather, or V_f and the response gradient, are skipped,
 *   and the gradient that is computed has the bits of the joint call.  Both are written in full.
 *   ws      scratch of golf_stft_filter_frames_bwd_workspace_bytes() bytes (0 for a refused geometry), 256-aligned: the gv_f.
 * Refused before any launch: n not a power of two in [64, 2048] or a call too large (GOLF_EUNSUPPORTED); n < 2*hop, T <= n/2,
 * null pointers, row strides below the row length (GOLF_EINVAL); a missing, short or misaligned workspace (GOLF_EWORKSPACE).
 * Two launches (frames, then the gather; Ty = 0 writes zeros and transforms nothing), no allocation, no host<->device
 * synchronisation, capturable in a hipGraph.  v_f and gu_f are transformed separately (a packed v + i*gu transform would
 * round GU_f relative to the signal's magnitude); every sum runs in a fixed order: the gradients are bit-reproducible. */
size_t golf_stft_filter_frames_bwd_workspace_bytes(int B, int T, int F, int n_fft, int hop);
int golf_stft_filter_frames_bwd_f32(const float* gy, int64_t gy_stride, const float* x, int64_t x_stride, const float* h,
                                    int h_kind, const float* window, float* g_x, int64_t g_x_stride, float* g_h, int B, int T,
                                    int F, int n_fft, int hop, void* ws, size_t ws_bytes, void* stream);

/* Custom backward of the above (what autograd computes in the reference through conv_transpose1d, lfilter, unfold,
 * the zero pad and the gain product; closed form in oracle/golf_oracle.py::lti_frames_ola_backward, pinned by
 * tests/golden/g15):  g_q = gy/norm;  u_f = the frame's all-pole recursion run backwards in time on window*g_q;
 *     g_a[f,i] = -sum_k u_f[k]*y_f[k-1-i];   g_x = overlap-add of the u_f;   g_ex = g_x*G;   g_gain = up^T(g_x*ex).
 *   ws_fwd = the forward's workspace, unmodified (it holds the filtered frames y_f);
 *   ws     = scratch of golf_lti_frames_bwd_workspace_bytes();
 *   g_ex (B, g_ex_len >= Tx) is fully written (zeros past Tx and past sample (F-1)*hop: ABI 5); g_gain (B,F) and
 *   g_a (B,F,M) are fully overwritten.  Any shape the forward accepts: the ring chain (quad adjoint, wave-per-frame g_a)
 *   where a ring exists, W % ring width == 0 and the g_a kernel's LDS rows fit (16*(2*W + ring + 6) <= 65536 bytes); the
 *   wave-per-frame adjoint and the tiled g_a kernel of lpc_ff_any.hip everywhere else.  Every sum runs in a fixed order on
 *   both chains: the gradients are bit-reproducible. */
size_t golf_lti_frames_bwd_workspace_bytes(int B, int Tx, int F, int M, int hop, int W);
int golf_lti_frames_ola_bwd_f32(const float* gy, int64_t gy_stride, const float* ex, int64_t ex_stride,
                                const float* gain, const float* a, const float* window, float* g_ex,
                                int64_t g_ex_stride, int g_ex_len, float* g_gain, float* g_a, int B, int Tx, int F,
                                int M, int hop, int W, int Ty, const void* ws_fwd, void* ws, size_t ws_bytes,
                                void* stream);

/* a-6: the same frame-wise synthesis with the all-pole filter given as a CASCADE of K second-order sections.
 * Replaces BatchSecondOrderLPCSynth.forward, models/lpc.py:94-131 (pad, unfold, K successive torchaudio lfilter calls
 * with a = biquads[...,k,:] and b = [1,0,0], windowed overlap-add, normalisation).
 *   biquads (B,F,K,3) = (a0,a1,a2) per section, K <= 16;  frames of W samples every hop of the signal zero-padded by
 *   `pad` on both sides (the reference class uses (W-hop)/2; LTVMinimumPhaseFilter's convention is W/2);
 *   gain_mode 1: frame f is scaled by gain[b,f] (the reference class); 0: ex is multiplied by up(gain) first.
 *   nfr = (Tx + 2*pad - W)/hop + 1 <= F,  Ty = (nfr-1)*hop + W - 2*pad;  ws: golf_lti_frames_workspace_bytes(). */
int golf_biquad_frames_ola_fwd_f32(const float* ex, int64_t ex_stride, const float* gain, const float* biquads,
                                   const float* window, float* y, int64_t y_stride, int B, int Tx, int F, int K,
                                   int hop, int W, int pad, int gain_mode, int Ty, void* ws, size_t ws_bytes,
                                   void* stream);

/* Backward of the cascade (the reference's is autograd through its K lfilter calls, models/lpc.py:115-118; closed form in
 * oracle/golf_oracle.py::biquad_frames_ola_backward, pinned by the reference's own gradients in tests/golden/g26):
 *   g_q = gy / norm (the caller divides: norm = overlap-add of the window);  per frame, u_K = window * g_q and
 *   u_{k-1} = section k run BACKWARDS in time on u_k;  g_biquads[b,f,k,i] = -sum_n u_{k-1}[n] * y_k[n-i] (y_k = the section's
 *   output, recomputed);  the frames' u_0 are overlap-added:
 *   gain_mode 1: g_ex = that sum (each frame scaled by its gain), g_gain_frames[b,f] = sum_n u_0[n] * x_f[n];
 *   gain_mode 0: g_ex = sum * up(gain), and gx_ex (B,Tx) = sum * ex for the caller to fold onto the gain frames (up^T).
 *   g_ex (B,Tx), g_biquads (B,F,K,3) are fully overwritten; ws: golf_biquad_frames_bwd_workspace_bytes(). */
size_t golf_biquad_frames_bwd_workspace_bytes(int B, int Tx, int F, int K, int hop, int W, int pad);
int golf_biquad_frames_ola_bwd_f32(const float* gq, int64_t gq_stride, const float* ex, int64_t ex_stride,
                                   const float* gain, const float* biquads, const float* window, float* g_ex,
                                   int64_t g_ex_stride, float* g_gain_frames, float* g_biquads, float* gx_ex,
                                   int B, int Tx, int F, int K, int hop, int W, int pad, int gain_mode, int Ty,
                                   void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a-2: control transform of the LPC filters, logits -> direct-form coefficients.
 * Replaces rc2lpc(tanh(logits) * max_abs_value), models/filters.py:91-97 + models/utils.py:581-593 (a Python loop of
 * M-1 Levinson step-up iterations A_n = [A_{n-1}, 0] + k_n * flip([A_{n-1}, 0]), ~100 tiny kernels) by one kernel.
 *   logits (N, M) with N = B*F frames, contiguous;  a (N, M) = a_1..a_M;  M <= 64;
 *   apply_tanh != 0: k = tanh(logits) * max_abs;  0: k = logits (reflection coefficients given directly).
 * Backward: g_logits (N, M) from g_a (N, M) (the adjoint of the step-up, through the tanh when apply_tanh). */
int golf_rc2lpc_fwd_f32(const float* logits, float* a, int64_t N, int M, float max_abs, int apply_tanh,
                        void* stream);
int golf_rc2lpc_bwd_f32(const float* logits, const float* g_a, float* g_logits, int64_t N, int M, float max_abs,
                        int apply_tanh, void* stream);

/* The biquad parameterisations of the ISMIR'23 configs, logits (N, 2K) -> K second-order sections -> their product in
 * direct form a (N, 2K).  Replaces get_logits2biquads(rep)(logits) + biquads2lpc, models/utils.py:487-525 and :444-484
 * (models/filters.py:71-81), 112 kernels in PyTorch ops.  rep: 0 "coef", 1 "conj", 2 "real"; 2K <= 64. */
int golf_sos2lpc_fwd_f32(const float* logits, float* a, int64_t N, int K, float max_abs_pole, int rep, void* stream);
int golf_sos2lpc_bwd_f32(const float* logits, const float* g_a, float* g_logits, int64_t N, int K, float max_abs_pole,
                         int rep, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a-8/a-9: indexed glottal-flow wavetable oscillator.
 * Replaces IndexedGlottalFlowTable.forward, models/synth.py:213-263 (table blend, phase/oversampling,
 * linear upsample, fp32 cumsum, %1, GlottalFlowTable.generate = F.grid_sample bilinear
 * models/synth.py:124-177, * rsqrt(phase), kazane.Decimate(oversampling)).
 *   phase (B,Tp) phase increment [cycles/sample] at hop phase_hop; wsel (B,Fw) in [0,1] at hop w_hop;
 *   table (n_tab, L).  Oversampled length N = (Tp-1)*phase_hop*os + 1 (N = Tp if phase_hop*os==1).
 *   pre (B,N) (optional, may be NULL) = the signal handed to the decimator;
 *   out (B,Tout): os==1 -> out = pre (Tout = N); os>1 -> strided FIR with `taps` (K odd),
 *   Tout = (N-1)/os + 1.
 *   The running phase is accumulated exactly (64-bit fixed point; the reference uses an fp32
 *   cumsum; parity is against the float64 oracle).
 *   addend (B, Tadd rows of stride addend_stride; optional, may be NULL; os > 1 only): out[b,o] += addend[b,o] for
 *   o < Tadd — the `harm_osc + noise_filter(noise)` of SourceFilterSynth.forward, models/sf.py:53-56, fused into the
 *   decimator's epilogue (one full-tensor round trip and one launch less per step). */
size_t golf_glottal_osc_workspace_bytes(int B, int Tp, int phase_hop, int Fw, int w_hop, int L, int os);

/* ABI 6: the decimation taps laid out for the matrix pipe, ONCE per tap set instead of once per step.  The fused oscillator
 * (os = 4, phase at hop 1, power-of-two table) multiplies the 4x oversampled signal by Toeplitz fragments of the taps
 * (v_mfma_f32_16x16x4_f32); they are a function of the taps alone -- kazane.Decimate's kernel is a constant buffer of the module,
 * models/synth.py:208-211 -- so a caller prepares them when the taps change and hands them to every forward / backward as
 * `tap_frags`.  NULL is always allowed: the call then lays them out itself (one small launch more).  A backward with
 * GOLF_OSC_WS_KEPT takes the same `tap_frags` its forward took.  _bytes returns 0 where the fused path does not apply. */
size_t golf_glottal_osc_tap_fragments_bytes(int K, int os);
int golf_glottal_osc_tap_fragments_f32(const float* taps, int K, int os, void* frags, size_t frags_bytes, void* stream);

/* equal_energy | GOLF_OSC_THROUGHPUT (ABI 6, forward only): the caller keeps SEVERAL batches in flight on the device (cf.
 * GOLF_SS_THROUGHPUT): below a device-filling batch the phase scan then runs as a small launch of its own in front of the
 * fused kernel instead of inside it -- measured cheaper by ~1.3 us per B = 32 step with four batches in flight, equal for a
 * lone batch, 3 % dearer at B = 16 384 (where the flag changes nothing).  Results are bit-identical either way. */
#define GOLF_OSC_THROUGHPUT 4
/* Round 6: ONE launch for the fused configuration.  The running phase is a single-pass scan inside the kernel (decoupled
 * look-back over tagged entries in `ws`; no totals launch, the phase is read once) -- the workspace may hold anything on entry
 * (no zero-fill is required, stale entries of earlier launches never validate) but must not be shared by launches in flight
 * at the same time. */
int golf_glottal_osc_fwd_f32(const float* phase, int64_t phase_stride, int Tp, int phase_hop,
                             const float* wsel, int Fw, int w_hop,
                             const float* table, int n_tab, int L,
                             int os, int equal_energy, const float* taps, int K,
                             float* pre, float* out, int64_t out_stride, int B, int Tout,
                             void* ws, size_t ws_bytes, void* stream,
                             const float* addend, int64_t addend_stride, int Tadd, const void* tap_frags);

/* ABI 6 (round 6): the source and the end filter's transition maps in ONE launch -- SourceFilterSynth.forward's
 * `harm_osc(...) + noise` followed by `end_filter(...)`, models/sf.py:47-64, where the filter's chunk transition maps
 * (golf_ltv_allpole_transitions_f32) depend on the coefficients only and not on the source.
 *   == golf_glottal_osc_fwd_f32(phase .. tap_frags; pre = NULL)  then
 *      golf_ltv_allpole_transitions_f32(a, B, T, F, M, hop, ss_ws, ss_ws_bytes, ss_flags, stream)
 * bit for bit; as one grid (oscillator workgroups beside the transition-map waves: a lone B = 32 batch ~42 us instead of
 * 6 + 18 + 38) when ss_flags holds GOLF_SS_FAST_TRANSITIONS | GOLF_SS_MAPS_ONLY, the oscillator's fused configuration applies
 * and the filter runs on its 24-sample ring with 22 taps (lpc_order 19 .. 22, hop % 24 == 0); as the two calls otherwise.
 * The caller then runs golf_ltv_allpole_fwd_f32(out as ex, .., ss_ws, ss_flags | GOLF_SS_HAVE_TRANSITIONS).
 * osc_ws / ss_ws: the two calls' workspaces (golf_glottal_osc_workspace_bytes / golf_ltv_allpole_workspace_bytes_ex). */
int golf_source_transitions_f32(const float* phase, int64_t phase_stride, int Tp, int phase_hop,
                                const float* wsel, int Fw, int w_hop,
                                const float* table, int n_tab, int L,
                                int os, int equal_energy, const float* taps, int K,
                                float* out, int64_t out_stride, int B, int Tout,
                                void* osc_ws, size_t osc_ws_bytes,
                                const float* addend, int64_t addend_stride, int Tadd, const void* tap_frags,
                                const float* a, int T, int F, int M, int hop,
                                void* ss_ws, size_t ss_ws_bytes, int ss_flags, void* stream);

/* Backward w.r.t. table_select_weight only (phase is data in GOLF training: train_with_true_f0,
 * cfg/ae/vctk.yaml:72):  g_wsel (B,Fw) overwritten.  ws = a workspace of the forward's size.
 * equal_energy | GOLF_OSC_WS_KEPT (ABI 5): the caller vouches that `ws` is exactly as golf_glottal_osc_fwd_f32 left it for
 * these same arguments with pre == NULL (an autograd node that saved it): the backward then reuses the forward's phase tile
 * totals and tap fragments instead of recomputing them (one launch of three less, ~6 us at B = 32).  Without the flag nothing
 * is assumed about the workspace's contents. */
#define GOLF_OSC_WS_KEPT 2
int golf_glottal_osc_bwd_wsel_f32(const float* g_out, int64_t g_out_stride,
                                  const float* phase, int64_t phase_stride, int Tp, int phase_hop,
                                  const float* wsel, int Fw, int w_hop,
                                  const float* table, int n_tab, int L,
                                  int os, int equal_energy, const float* taps, int K,
                                  float* g_wsel, int B, int Tout,
                                  void* ws, size_t ws_bytes, void* stream, const void* tap_frags);

/* Generic wavetable lookup = GlottalFlowTable.generate, models/synth.py:124-177 (F.grid_sample bilinear over
 * (control frame, phase)), for arbitrary per-frame tables (B,K,L) at hop hop_t and a given wrapped phase (B,N) in [0,1):
 * what WeightedGlottalFlowTable (:266-294), WrappedPhaseDownsampledIndexedGlottalFlowTable (:343-375) and
 * IndexedGlottalFlowTable with a differentiable phase / phase_offset / trainable table (:59-70,:213-218) reduce to.
 *   out[b,n] = bilerp(T[b], row n/hop_t (frames beyond K-1 replicate the last), column wrapped*L (wraps to column 0))
 * Backward: g_wrapped (B,N) and/or g_tables (B,K,L) (either may be NULL; both are fully overwritten). */
int golf_wavetable_lookup_fwd_f32(const float* wrapped, int64_t wrapped_stride, const float* tables, int K, int L,
                                  int hop_t, float* out, int64_t out_stride, int B, int N, void* stream);
int golf_wavetable_lookup_bwd_f32(const float* g_out, int64_t g_out_stride, const float* wrapped, int64_t wrapped_stride,
                                  const float* tables, int K, int L, int hop_t, float* g_wrapped,
                                  int64_t g_wrapped_stride, float* g_tables, int B, int N, void* stream);

/* The running phase of those general table oscillators (ABI 3):
 *   wrapped[b,n] = frac( cumsum(up(phase / os))[n] + phase_offset[b,n] ),   n < N <= (Tp-1)*phase_hop*os + 1
 * Replaces F.interpolate + torch.cumsum (float32 in the reference) + % 1 of IndexedGlottalFlowTable.forward,
 * models/synth.py:239-255, with the exact 64-bit fixed-point prefix of the fused oscillator.  phase_offset (B,>=N) at the
 * fine rate, or NULL.  The gradient w.r.t. phase is the transposed upsampling of the reverse cumulative sum (host). */
size_t golf_phase_accumulate_workspace_bytes(int B, int Tp);
int golf_phase_accumulate_f32(const float* phase, int64_t phase_stride, int Tp, int phase_hop, int os,
                              const float* phase_offset, int64_t offset_stride, float* wrapped, int64_t wrapped_stride,
                              int B, int N, void* ws, size_t ws_bytes, void* stream);

/* Streaming oscillator (additive in ABI 6): golf_glottal_osc_fwd_f32's fine-rate signal (before decimation) for the
 * fine samples of coarse phase samples j0 .. j0+nseg-1, from a carried phase:
 *   phase  (B, >= nseg+1) rows of stride phase_stride: phase[b][i] = p[b][j0+i] (p[j0+nseg] closes the last segment)
 *   acc    (B) uint64 DEVICE words, Q0.64 cycles: on entry the exact phase before fine sample j0*P (P = phase_hop*os), on
 *          return the phase before sample (j0+nseg)*P -- the same integer sums as the one-shot scan, so any split of the
 *          track into calls accumulates the one-shot's phase bit for bit
 *   final_point 1: also the utterance's last fine sample, k = 0 of coarse sample j0+nseg (the one-shot's (Tp-1)*P)
 *   wsel   (B, >= nw) rows of stride wsel_stride: rows w_first .. w_first+nw-1 of the table-select track at w_hop output
 *          samples; rows past the last given one repeat it (the one-shot's last frame at the utterance's end), rows before
 *          w_first must not be needed
 *   pre    (B, nseg*P + final_point) stride pre_stride: the fine samples (table blend, bilinear lookup, equal_energy scale)
 *   wrapped (optional, may be NULL; same shape and stride as pre): frac of the inclusive phase as fp32, bit-identical to
 *          golf_phase_accumulate_f32's output at the same fine samples
 * Decimation is left to the caller (golf_decimate_fir_f32 over a window that carries (K-1)/2 fine samples of context). */
int golf_glottal_osc_stream_f32(const float* phase, int64_t phase_stride, int nseg, int final_point, int phase_hop, int os,
                                const float* wsel, int64_t wsel_stride, int nw, int64_t w_first, int w_hop,
                                const float* table, int n_tab, int L, int equal_energy, int64_t j0, uint64_t* acc,
                                float* pre, int64_t pre_stride, float* wrapped, int B, void* stream);

/* The oscillator's decimator on its own (kazane.Decimate(os) stand-in, models/synth.py:208,262; taps are an input):
 *   out[b,o] = sum_k taps[k] * x[b, o*os + k - (K-1)/2], zero padded, Tout = (N-1)/os + 1, K odd, os in [2,64];
 * golf_decimate_fir_adj_f32 is its transpose (g_x (B,N) dense, fully overwritten). */
int golf_decimate_fir_f32(const float* x, int64_t x_stride, int N, const float* taps, int K, int os, float* out,
                          int64_t out_stride, int B, int Tout, void* stream);
int golf_decimate_fir_adj_f32(const float* g_out, int64_t g_out_stride, int Tout, const float* taps, int K, int os,
                            float* g_x, int N, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f-1: zero-phase FIR noise filter of every GOLF decoder.
 * Replaces LTVZeroPhaseFIRFilter.forward, models/filters.py:340-384:
 *     kernel = fftshift(irfft(exp(log_mag))) * window                    (filters.py:294-306)
 *     frames of N+hop-1 samples of the zero-padded excitation every hop  (filters.py:357-364)
 *     one cross-correlation per frame with that frame's kernel (grouped F.conv1d, filters.py:371-383)
 *
 *   N = 2*(n_mag-1) taps, P = (N-1)/2,  nfr = min((T + 2P - (N+hop-1))/hop + 1, F) frames,
 *   y[b, f*hop+n] = sum_{k<N} xp[b, f*hop+n+k] * kernel[b,f,k],  xp = ex zero-padded by P both sides,
 *   output length nfr*hop (golf_ltv_fir_frames_length; -1 if T is shorter than one frame span).
 *
 * The inverse real FFT of a zero-phase spectrum is a cosine transform: a dense (B*F, n_mag) x (n_mag, n_mag)
 * contraction, run on the matrix cores in exact fp32.  Its constant matrix (`basis`, both orientations) is built
 * once per n_mag by golf_zero_phase_fir_basis_f32 into a caller-owned buffer of golf_zero_phase_fir_basis_bytes().
 * Kernel rows live in a (B*F, row_stride) buffer, row_stride = golf_zero_phase_fir_row_stride(n_mag) >= N floats
 * (taps [N, row_stride) are written as zeros); golf_ltv_fir_frames_* accept any per-frame kernels in that layout.
 * ------------------------------------------------------------------------------------------- */
int golf_zero_phase_fir_row_stride(int n_mag);
size_t golf_zero_phase_fir_basis_bytes(int n_mag);
int golf_zero_phase_fir_basis_f32(int n_mag, void* basis, size_t basis_bytes, void* stream);

/* log_mag (G, n_mag), window (N) -> kern (G, row_stride);  G = B*F */
int golf_zero_phase_fir_kernels_f32(const float* log_mag, const float* window, const void* basis, float* kern,
                                    int G, int n_mag, void* stream);
/* g_kern (G, row_stride) -> g_log_mag (G, n_mag): the adjoint of window * fftshift * irfft, times exp(log_mag) */
int golf_zero_phase_fir_kernels_bwd_f32(const float* g_kern, const float* log_mag, const float* window,
                                        const void* basis, float* g_log_mag, int G, int n_mag, void* stream);

int golf_ltv_fir_frames_length(int T, int F, int N, int hop);
/* ex (B, >=T) stride ex_stride; kern (B*F, kern_row_stride), zero in [N, ceil4(N)); y (B, nfr*hop) stride y_stride.
 * frame0 (normally 0): output frame f is filtered with kernel row f + frame0, nfr = min(frames in T, F - frame0) —
 * what the sample-wise variant (LTVZeroPhaseFIRFilterPrecise, models/filters.py:286-337: kernels interpolated between
 * frames f and f+1) needs for its second term.  N <= 3836: a wave stages 256 + ceil4(N) + 4 floats and the four waves of
 * a workgroup share 64 KiB of dynamic LDS; a longer kernel is GOLF_EUNSUPPORTED (checked on the host, nothing is launched). */
int golf_ltv_fir_frames_fwd_f32(const float* ex, int64_t ex_stride, const float* kern, int kern_row_stride, float* y,
                                int64_t y_stride, int B, int T, int F, int N, int hop, int frame0, void* stream);
/* gy (B, nfr*hop).  g_ex (B,T) and g_kern (B*F, kern_row_stride; rows of unused frames and the padding taps [N, kern_row_stride) zeroed) are fully
 * overwritten; either may be NULL to skip it.  Requires hop % 4 == 0 and, by the same 64 KiB of LDS (the frame's hop gradient
 * samples are the packed taps here), hop <= 3836: GOLF_EUNSUPPORTED otherwise. */
int golf_ltv_fir_frames_bwd_f32(const float* gy, int64_t gy_stride, const float* ex, int64_t ex_stride,
                                const float* kern, int kern_row_stride, float* g_ex, int64_t g_ex_stride,
                                float* g_kern, int B, int T, int F, int N, int hop, int frame0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Minimum-phase FIR filter: the causal twin of f-1 (same magnitude response, impulse response from tap 0, no lookahead).
 * Replaces LTVMinimumPhaseFIRFilterPrecise.get_minimum_phase_fir + windowing, models/filters.py:203-221 (with
 * hilbert, models/utils.py:557-574):
 *     L_sym = [log_mag, flip(log_mag)[1:-1]];  theta = -Im hilbert(L_sym);  kernel = Re ifft(exp(L_sym + j theta)) * window
 * as two dense real contractions on the matrix cores in exact fp32 (N = 2*(n_mag-1), w = 1 at bins 0 and N/2, else 2):
 *     theta = log_mag @ S^T,   kernel = (e^L cos theta) @ C - (e^L sin theta) @ Sn,
 *     C[k][m] = w_k cos(2 pi k m / N) / N,  Sn[k][m] = w_k sin(2 pi k m / N) / N,  S = the Hilbert transform on the half spectrum.
 * `basis` holds S, C and Sn in both orientations, built once per n_mag into a caller-owned buffer of
 * golf_min_phase_fir_basis_bytes().  `window` is a vector of N taps (the reference's windowing(), filters.py:216-221, is
 * window_fn(N) with its first N/2 entries set to 1: the caller builds it).  Rows go to the (G, row_stride) layout of
 * golf_zero_phase_fir_row_stride(n_mag), taps [N, row_stride) written as zeros.  One workgroup keeps its rows in LDS from
 * the log magnitudes to the finished taps: GOLF_EUNSUPPORTED where they do not fit (forward n_mag > 640, backward > 512).
 * Nothing is allocated, nothing synchronises.
 * ------------------------------------------------------------------------------------------- */
size_t golf_min_phase_fir_basis_bytes(int n_mag);
int golf_min_phase_fir_basis_f32(int n_mag, void* basis, size_t basis_bytes, void* stream);
/* log_mag (G, n_mag), window (N) -> kern (G, row_stride);  G = B*F */
int golf_min_phase_fir_kernels_f32(const float* log_mag, const float* window, const void* basis, float* kern, int G,
                                   int n_mag, void* stream);
/* g_kern (G, row_stride) -> g_log_mag (G, n_mag); theta is recomputed from log_mag */
int golf_min_phase_fir_kernels_bwd_f32(const float* g_kern, const float* log_mag, const float* window, const void* basis,
                                       float* g_log_mag, int G, int n_mag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mel-cepstral filter design: mel cepstra -> complex minimum-phase response rows, the design step of LTVMLSAFilter2
 * (models/filters.py:626-684; gamma = 0, the plain mel cepstrum, only).  The package's own definition, exact in float64,
 * with N = n_fft, M = order, bins k = 0 .. N/2, w_k = 2 pi k / N:
 *     theta_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k)              the all-pass phase warp; theta_0 = 0, theta_{N/2} = pi
 *     L_k     = sum_{m=0..M} mc[m] (cos(m theta_k) - j sin(m theta_k))       the natural logarithm of H
 *     H_k     = exp(Re L_k) (cos(Im L_k) + j sin(Im L_k))
 * The warped cepstrum is causal, so Im L is the minimum phase.  The reference truncates the warped cepstrum at order N/2
 * and takes the phase from a discrete Hilbert transform instead; the two agree to 5e-15 in L for N >= 256 with M <= 64 and
 * alpha <= 0.77, and differ where the truncated tail is not negligible (2e-2 at N 128, 0.2 at N 64 with M 24, alpha 0.46):
 * below N 256 this definition is the specification.
 * Rows are (R, N/2+1, 2) interleaved complex -- the h_kind 1 layout of golf_stft_filter_frames_* -- with Im H exactly 0 at
 * bins 0 and N/2.  A row's bits depend on its own mc row and the basis only (not on R, the row's position or its
 * neighbours), which is what makes a streamed decoder equal the one-shot one bit for bit.
 * `basis` holds cos(m theta_k) and sin(m theta_k) as fp32 values rounded once from a float64 evaluation (the sine exactly 0
 * at bins 0 and N/2), built once per (n_fft, order, alpha) into a caller-owned buffer of golf_mlsa_response_basis_bytes()
 * (0 for an unsupported geometry).
 * Backward, with g_h in torch's complex convention (d/d re + j d/d im), P + jQ = conj(g_h_k) H_k:
 *     g_mc[m] = sum_{k=0..N/2} (P_k cos(m theta_k) + Q_k sin(m theta_k))
 * H is recomputed from mc; the bins are summed in a fixed order without atomics: bit-reproducible.
 * Refused before any launch: null pointers (GOLF_EINVAL), n_fft not a power of two in [64, 2048] or order outside [0, 64]
 * (GOLF_EUNSUPPORTED), |alpha| >= 1 (GOLF_EINVAL), a basis buffer shorter than golf_mlsa_response_basis_bytes()
 * (GOLF_EWORKSPACE), R < 0 (GOLF_EINVAL).  R = 0 does nothing.  Nothing is allocated, nothing synchronises.
 * ------------------------------------------------------------------------------------------- */
size_t golf_mlsa_response_basis_bytes(int n_fft, int order);
int golf_mlsa_response_basis_f32(int n_fft, int order, double alpha, void* basis, size_t basis_bytes, void* stream);
/* mc (R, order+1) -> h (R, n_fft/2+1, 2) */
int golf_mlsa_response_rows_f32(const float* mc, const void* basis, size_t basis_bytes, float* h, int R, int n_fft, int order,
                                void* stream);
/* g_h (R, n_fft/2+1, 2), mc (R, order+1) -> g_mc (R, order+1) */
int golf_mlsa_response_rows_bwd_f32(const float* g_h, const float* mc, const void* basis, size_t basis_bytes, float* g_mc, int R,
                                    int n_fft, int order, void* stream);

/* Causal frame FIR, replaces LTVMinimumPhaseFIRFilter.forward, models/filters.py:270-283 (left pad by N-1, unfold
 * N+hop-1 samples every hop, correlate each frame with its flipped kernel):
 *     y[b, f*hop+n] = sum_{j<N} kernel[b,f,j] * ex[b, f*hop+n-j],   nfr = min(T / hop, F - frame0) frames,
 * output length nfr*hop (golf_ltv_fir_frames_causal_length; -1 if T < hop).  Arguments, kernel-row layout, frame0 and
 * the backward's hop % 4 == 0 are those of golf_ltv_fir_frames_{fwd,bwd}_f32. */
int golf_ltv_fir_frames_causal_length(int T, int F, int N, int hop);
int golf_ltv_fir_frames_causal_fwd_f32(const float* ex, int64_t ex_stride, const float* kern, int kern_row_stride,
                                       float* y, int64_t y_stride, int B, int T, int F, int N, int hop, int frame0,
                                       void* stream);
int golf_ltv_fir_frames_causal_bwd_f32(const float* gy, int64_t gy_stride, const float* ex, int64_t ex_stride,
                                       const float* kern, int kern_row_stride, float* g_ex, int64_t g_ex_stride,
                                       float* g_kern, int B, int T, int F, int N, int hop, int frame0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f-2: LTI FIR shared by the whole batch — the room filter after the end filter.
 * Replaces LTIAcousticFilter.forward, models/filters.py:426-449 (pad + F.conv1d with one learnable kernel):
 *     y[b,t] = sum_{n<ntaps} taps[n] * ex[b, t - lead + n],   ex = 0 outside [0,T)
 *   (the reference's y = ex + conv(pad(ex[:, :-1], (K,0)), kernel) is taps = [kernel, 1], lead = K).
 *   ntaps must be a multiple of 4 (pad with zero taps), 0 <= lead < ntaps, |ntaps| <= 3836 (64 KiB of dynamic LDS per
 *   workgroup; more is GOLF_EUNSUPPORTED, checked on the host before any launch; the taps gradient has no such limit).
 *   The adjoint w.r.t. ex is the same call with the taps reversed and lead' = ntaps-1-lead; ABI 5: ntaps < 0 applies the
 *   |ntaps| taps in reverse order, so the adjoint needs no flipped copy of them.
 * golf_lti_fir_taps_grad_f32: g_taps[n] = sum_{b,t} gy[b,t] * ex[b, t - lead + n]  (deterministic two-stage sum).
 * ------------------------------------------------------------------------------------------- */
int golf_lti_fir_f32(const float* ex, int64_t ex_stride, const float* taps, int ntaps, int lead, float* y,
                     int64_t y_stride, int B, int T, void* stream);
size_t golf_lti_fir_taps_grad_workspace_bytes(int B, int T, int ntaps);
int golf_lti_fir_taps_grad_f32(const float* gy, int64_t gy_stride, const float* ex, int64_t ex_stride, float* g_taps,
                               int ntaps, int lead, int B, int T, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a-12: filtered-noise-band generator.  Replaces NoiseBand.forward, models/noise.py:114-124:
 *     out[b,t] = sum_k noise_bands[k][(t + offsets[b,k]) mod Lb] * up(exp(log_gain))[b,t,k]
 *   noise_bands (K, Lb) one loopable period per band (Lb a power of two; built at init by the host module as
 *   models/noise.py:141-213 does), offsets (B,K) int32 in [0,Lb) (the random start per utterance and band),
 *   log_gain (B,F,K) at hop `hop`, out (B,T), T <= (F-1)*hop+1.  The (B,K,T) gather and the (B,T,K) upsampled gains of
 *   the reference are never formed.  Backward w.r.t. log_gain (g_log_gain (B,F,K) fully overwritten).
 * ------------------------------------------------------------------------------------------- */
size_t golf_noise_band_workspace_bytes(int B, int F, int K);
int golf_noise_band_fwd_f32(const float* noise_bands, int Lb, const int* offsets, const float* log_gain, int F, int hop,
                            float* out, int64_t out_stride, int B, int T, int K, void* stream);
int golf_noise_band_bwd_f32(const float* g_out, int64_t g_out_stride, const float* noise_bands, int Lb,
                            const int* offsets, const float* log_gain, int F, int hop, float* g_log_gain, int B, int T,
                            int K, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a-11: harmonic oscillator bank — the source of the DDSP / NHV / WORLD / MLSA / SawSing / PULF baselines.
 * Replaces HarmonicOscillator.forward, models/synth.py:403-446, and what AdditiveSynthesizer (:449-468),
 * SawToothOscillator (:486-504) and AdditivePulseTrain (:526-547) feed it:
 *     p = up(phase)  [cycles/sample, linear upsampling from phase_hop];   Phi = inclusive cumsum of p
 *     out[t] = sum_{h=1..H} [h*p(t) < 0.5] * amp(t,h) * sin(2 pi h Phi(t))
 *     amp(t,h) = up(A)[t,h] * up(tscale)[t] * hscale[h];  A (B,Fa,H) at amp_hop, tscale (B,Fs) at ts_hop, hscale (H):
 *     each may be NULL (= 1).  Tout = min of the upsampled lengths ((n-1)*hop+1) of phase, the given factors and
 *     phase_offset (below): whichever track is shortest ends the output.
 *   Limits, refused before any launch (GOLF_EUNSUPPORTED): H <= 4096; with amplitudes (256 / amp_hop + 4) * H * 4 <= 61440;
 *   and the forward / dphase launch's whole LDS request, 2080 + 4 * (((H+3) & ~3) + rows * H + (initial_phase ? 2 H : 0))
 *   bytes with rows = 256 / amp_hop + 3 (1 without amplitudes), <= 65536: e.g. H <= 59 at amp_hop 1, and with initial_phase
 *   H <= 2266 at amp_hop 256 and H <= 3965 without amplitudes.  _bwd_amp stages nothing and has no such limit.
 *   The (B,T,H) tensors of the reference are never formed; the phase is exact (64-bit fixed point, as in the
 *   wavetable oscillator), sin(h theta) by a rotation recurrence re-anchored from the exact phase every 32 harmonics.
 * Backward w.r.t. A (g_amp (B,Fa,H) fully overwritten); golf_harmonic_osc_dphase_f32 serves the gradient w.r.t. the phase.
 *   Optional phase terms (ABI 3; models/synth.py:434-440): harmonic h runs at h * (Phi + up(phase_offset)) + initial_phase[b,h];
 *   phase_offset (B,Fo) cycles at hop po_hop (linear upsampling; a track shorter than the others ends the output, as the
 *   reference's mixed-hop addition does; one that does not cover Tout samples is refused), initial_phase (B,H) cycles;
 *   either may be NULL.  d out / d phase_offset(t) is what golf_harmonic_osc_dphase_f32 returns.
 * ------------------------------------------------------------------------------------------- */
/* Fa = amplitude frames (0 if amp is NULL); sized for the forward and the backward */
size_t golf_harmonic_osc_workspace_bytes(int B, int Tp, int phase_hop, int Fa, int H);
int golf_harmonic_osc_fwd_f32(const float* phase, int64_t phase_stride, int Tp, int phase_hop,
                              const float* amp, int Fa, int amp_hop, const float* tscale, int Fs, int ts_hop,
                              const float* hscale, int H, float* out, int64_t out_stride, int B, int Tout,
                              void* ws, size_t ws_bytes, void* stream,
                              const float* phase_offset, int Fo, int po_hop, const float* initial_phase);
/* Streaming harmonic oscillator (additive in ABI 6): golf_harmonic_osc_fwd_f32's output samples of coarse phase segments
 * j0 .. j0+nseg-1, i.e. samples [j0*P, (j0+nseg)*P) with P = phase_hop, from a carried phase (golf_glottal_osc_stream_f32's
 * contract, without oversampling):
 *   phase  (B, >= nseg+1) rows of stride phase_stride: phase[b][i] = p[b][j0+i] (p[j0+nseg] closes the last segment)
 *   acc    (B) uint64 DEVICE words, Q0.64 cycles: on entry the exact phase before sample j0*P, on return the phase after the
 *          block -- the one-shot scan's integer segment sums, so any split accumulates the one-shot's phase bit for bit
 *   final_point 1: also the utterance's last sample, k = 0 of coarse sample j0+nseg (the one-shot's (Tp-1)*P)
 *   amp    (B, na, H) contiguous, NULL for none: rows a_first .. a_first+na-1 of the amplitude track at amp_hop;
 *   tscale (B, >= ns) rows of stride ts_stride, NULL for none: rows s_first .. s_first+ns-1 at ts_hop;
 *          a_end / s_end: -1 while the track is open, its total row count once known (the one-shot's clamps: the last
 *          sample interpolates segment end-2 with weight 1, a single row is held constant)
 *   hscale (H) or NULL; H <= 4096; out (B, nseg*P + final_point) of stride out_stride
 *   ws     scratch of 8*B*(nseg + final_point) bytes, 256-aligned
 * Every sample has the bits of golf_harmonic_osc_fwd_f32's sample at the same global index, for any split.  Refused before any
 * launch: windows that do not hold the rows the samples interpolate, a closed track that ends before the last sample, and
 * (GOLF_EUNSUPPORTED) the amplitude hops the one-shot refuses for LDS staging.  No phase_offset / initial_phase.  Two launches
 * (segment scan, render); none when nseg + final_point = 0.  No host<->device synchronisation. */
int golf_harmonic_osc_stream_f32(const float* phase, int64_t phase_stride, int nseg, int final_point, int phase_hop,
                                 const float* amp, int64_t a_first, int na, int64_t a_end, int amp_hop,
                                 const float* tscale, int64_t ts_stride, int64_t s_first, int ns, int64_t s_end, int ts_hop,
                                 const float* hscale, int H, int64_t j0, uint64_t* acc, float* out, int64_t out_stride, int B,
                                 void* ws, size_t ws_bytes, void* stream);
/* d out / d Phi(t) (Phi = the running phase in cycles): 2 pi sum_h [h p < 0.5] amp(t,h) h cos(2 pi h Phi(t)); the
 * gradient w.r.t. the phase input is the transposed upsampling of the reverse cumulative sum of g_out * this (host). */
int golf_harmonic_osc_dphase_f32(const float* phase, int64_t phase_stride, int Tp, int phase_hop,
                              const float* amp, int Fa, int amp_hop, const float* tscale, int Fs, int ts_hop,
                              const float* hscale, int H, float* out, int64_t out_stride, int B, int Tout,
                              void* ws, size_t ws_bytes, void* stream,
                              const float* phase_offset, int Fo, int po_hop, const float* initial_phase);
int golf_harmonic_osc_bwd_amp_f32(const float* g_out, int64_t g_out_stride, const float* phase, int64_t phase_stride,
                                  int Tp, int phase_hop, int Fa, int amp_hop, const float* tscale, int Fs, int ts_hop,
                                  const float* hscale, int H, float* g_amp, int B, int Tout,
                                  void* ws, size_t ws_bytes, void* stream,
                                  const float* phase_offset, int Fo, int po_hop, const float* initial_phase);

/* ---------------------------------------------------------------------------------------------
 * (e) multi-GPU: push-based exchange of the synthesised audio (north_star: "shards independent utterances across the 8
 * MI355X ... all-gathering only the synthesized audio").  The reference has no counterpart (it is single-device:
 * autoencode.py / test_rtf.py); what these replace is the torch.distributed.all_gather_into_tensor that
 * golf_amd.dist.gather_audio issues.  xGMI is point to point, so instead of a ring collective ONE kernel stores a
 * step's (rows, T) block into every peer's receive buffer (7 links at once, source read once), then publishes a
 * sequence number with system scope; the consumer waits for it in-stream.
 *   golf_peer_alloc     fine-grained device memory, zero-filled (receive buffers and flags: pollable while kernels run)
 *   golf_peer_export    -> GOLF_PEER_HANDLE_BYTES opaque bytes (hipIpcMemHandle_t) to send to the other processes
 *   golf_peer_open/close   map / unmap another process's buffer
 *   golf_peer_store_f32    src (rows, T) -> dst[i] (rows, T) for i < n_dst <= GOLF_MAX_PEERS; dst = HOST array of device
 *                          pointers (already offset to this rank's slot in each peer's buffer)
 *   golf_peer_signal_u32   *flags[i] = seq for i < n (release, system scope; ordered after this stream's stores)
 *   golf_peer_wait_u32     blocks the STREAM until flags[i*stride] >= seq for all i < n (signed distance: sequence numbers
 *                          may wrap), or sets *status (device int) to 1 + i after timeout_us -- never hangs the GPU
 * Used by golf_amd.dist.PeerStoreGather (bench.py --gather-mode peer-store).  Exercised with 2 processes on one GPU;
 * not yet measured on a multi-GPU node -- RCCL's all-gather remains the default exchange. */
#define GOLF_MAX_PEERS 16
#define GOLF_PEER_HANDLE_BYTES 64
int golf_peer_alloc(size_t bytes, void** ptr);
int golf_peer_free(void* ptr);
int golf_peer_export(void* ptr, void* handle64);
int golf_peer_open(const void* handle64, void** ptr);
int golf_peer_close(void* ptr);
int golf_peer_store_f32(const float* src, int64_t src_stride, int rows, int T, void* const* dst, int64_t dst_stride,
                        int n_dst, void* stream);
int golf_peer_signal_u32(void* const* flags, int n, uint32_t seq, void* stream);
int golf_peer_wait_u32(const uint32_t* flags, int n, int stride, uint32_t seq, int64_t timeout_us, int* status,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOLF_AMD_H */
