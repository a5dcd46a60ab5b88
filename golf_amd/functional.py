"""torch.autograd.Functions over the C ABI of libgolf_hip.so (include/golf_amd.h).

Plain tensors in, plain tensors out; AudioTensor bookkeeping lives in the nn.Modules.
Every function raises if the tensors are not ROCm-device tensors — no CPU path exists — and if they are not fp32, with one
exception: the sample-wise all-pole filter (``ltv_allpole_ss``, ``ltv_allpole_ss_blocks``) also takes float64 tensors, and
fp32 tensors with ``mode="fp64"``, and then runs its recursion in float64 on the device (csrc/lpc_any.hip).
"""
from __future__ import annotations

import dataclasses
import functools
import math

import torch

from . import _lib

__all__ = ["ltv_allpole_ss", "ltv_allpole_ss_blocks", "ltv_allpole_prepare", "ltv_inverse", "lpc_analysis", "source_filter_lpc", "f0_yin", "f0_candidates", "f0_viterbi", "f0_track", "f0_viterbi_stream",
           "f0_viterbi_stream_state", "harmonic_analysis", "harmonic_analysis_stream", "spectral_envelope", "spectral_envelope_stream", "ltv_residual", "ltv_residual_stream", "glottal_plan", "glottal_match", "GlottalPlan",
           "lti_frames_ola",
           "glottal_osc",
           "ss_output_length", "ss_has_f64", "ff_output_length", "osc_lengths", "PreparedTransitions", "ss_status",
           "zero_phase_fir_basis", "zero_phase_fir_kernels", "ltv_fir_frames", "zero_phase_fir_filter",
           "zero_phase_fir_filter_precise", "min_phase_fir_basis", "min_phase_window", "min_phase_fir_kernels",
           "min_phase_fir_filter", "min_phase_fir_filter_precise", "ltv_fir_frames_causal",
           "fir_frames_length", "lti_fir", "harmonic_osc", "biquad_frames_ola",
           "mel_cepstrum_response", "mel_cepstrum_response_torch", "mel_cepstrum_tables", "mel_cepstrum_basis",
           "mel_cepstrum_rows", "mel_cepstrum_kernel_takes"]

HAVE_TRANSITIONS = 1
FAST_TRANSITIONS = 2
TRAINING = 64            # GOLF_SS_TRAINING
MAPS_ONLY = 128          # GOLF_SS_MAPS_ONLY (ABI 4)
THROUGHPUT = 256         # GOLF_SS_THROUGHPUT (ABI 4)
ZERO_TAIL = 512          # GOLF_SS_ZERO_TAIL (ABI 5): the backward zeroes g_ex beyond the output length itself
OSC_THROUGHPUT = 4       # GOLF_OSC_THROUGHPUT (ABI 6): batches in flight -> the oscillator's phase scan as a launch of its own
OSC_WS_KEPT = 2          # GOLF_OSC_WS_KEPT (ABI 5): the oscillator's backward reuses the totals in the forward's saved workspace
FORK_TRANSITIONS = False
SPLIT_P1 = False   # diagnostic: bench.py --split-p1  # set True to run the transition kernel beside the zero-state pass (streams)
_side_streams = {}

# Mixed-precision entry (reference intent: models/synth.py:250-251 pins the phase cumsum to fp32 so that the decoder survives
# `precision: 16-mixed`).  The kernels are fp32: under torch.autocast every Function casts its floating-point inputs to fp32
# and runs with autocast off; the backward runs in the same mode.  Outside autocast a non-fp32 tensor is still an error.
_amp_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")


def _amp_no_grad(fn):
    """``_amp_fwd`` for an analysis that has no gradient, so that it needs no autograd.Function: under autocast the floating
    tensors on the device (float64 apart) become fp32 and ``fn`` runs with autocast off; every tensor is detached, so an input
    that requires grad is accepted and the outputs never do."""
    def prepared(v, amp):
        if not isinstance(v, torch.Tensor):
            return v
        if amp and v.is_floating_point() and v.is_cuda and v.dtype is not torch.float64:
            v = v.float()
        return v.detach()

    @functools.wraps(fn)
    def run(*args, **kwargs):
        amp = torch.is_autocast_enabled("cuda")
        args, kwargs = [prepared(v, amp) for v in args], {k: prepared(v, amp) for k, v in kwargs.items()}
        if not amp:
            return fn(*args, **kwargs)
        with torch.autocast("cuda", enabled=False):
            return fn(*args, **kwargs)

    return run


def _side_stream(device) -> "torch.cuda.Stream":
    """One extra HIP stream per device for the excitation-independent phase (transition matrices)."""
    key = torch.device(device).index
    if key is None:
        key = torch.cuda.current_device()
    s = _side_streams.get(key)
    if s is None:
        s = _side_streams[key] = torch.cuda.Stream(device=key)
    return s


class PreparedTransitions:
    """Handle returned by ltv_allpole_prepare: the workspace with the transition matrices in flight on the side
    stream, plus the shape key they are valid for."""

    def __init__(self, ws, key, stream, a, fast=False, training=False, maps_only=False):
        self.ws, self.key, self.stream, self.a, self.fast, self.training = ws, key, stream, a, fast, training
        self.maps_only = maps_only   # the matrices alone: the forward still runs their fix-up and the group composites


def ltv_allpole_prepare(a: torch.Tensor, hop: int, T: int, overlap: bool = False,
                        fast: bool = False, mode=None, training: bool = False,
                        maps_only: bool = False) -> PreparedTransitions:
    """Compute the transition matrices for coefficients ``a`` (B,F,M) and output length ``T`` ahead of the
    excitation; pass the handle to ltv_allpole_ss(..., prepared=handle) (e.g. to filter several signals with the
    same coefficients, or to start the most expensive, excitation-independent phase early).
    ``overlap=True`` launches on a second HIP stream that the forward joins right before its boundary scan.
    With the two-level boundary scan the group composites (which need only the matrices) are computed here as well.
    Off by default: the HIP fork/join (two event record/wait pairs) measured ~25 us of latency on ROCm 7.2 -- more than the
    ~20 us of the transition kernel that the oscillator can hide at B = 32 (round 3: one batch alone 161 us forked vs 137 us
    on one stream; training 370 vs 283) -- and with several batches in flight the chip is full either way.  It pays when
    much more work precedes the filter on the main stream than the join costs (a long encoder).
    ``fast=True`` computes the fp32 matrices of the inference path; ``training=True`` (implied by ``fast=False``) also keeps
    what the backward reads, so the handle serves a forward whose gradients are needed.
    ``maps_only=True`` (with ``fast``): only the transition matrices; the forward then runs what the boundary scan still
    needs from them (fix-up of ill-conditioned matrices, group composites) in the launch of its zero-state pass."""
    _lib.require_device(a)
    lib = _lib.load()
    a = a.detach().contiguous()
    B, F, M = a.shape
    maps_only = bool(maps_only and fast)
    flags = (SS_MODES[mode] | (FAST_TRANSITIONS if fast else 0) | (TRAINING if (fast and training) else 0)
             | (MAPS_ONLY if maps_only else 0))
    ws = _workspace(lib.golf_ltv_allpole_workspace_bytes_ex(B, T, F, M, hop, flags), a.device)
    cur = torch.cuda.current_stream(a.device)
    side = None
    if overlap:
        side = _side_stream(a.device)
        side.wait_stream(cur)  # `a` (and the fresh workspace) are ordered after the current stream's work
        ws.record_stream(side)
        a.record_stream(side)
    rc = lib.golf_ltv_allpole_transitions_f32(a.data_ptr(), B, T, F, M, hop, ws.data_ptr(), ws.numel(),
                                              flags, (side or cur).cuda_stream)
    _lib.check(rc, "golf_ltv_allpole_transitions_f32")
    return PreparedTransitions(ws, (B, T, F, M, hop, a.data_ptr(), a._version, SS_MODES[mode]), side, a, fast,
                               training or not fast, maps_only)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """2-D tensor with unit inner stride (row stride may exceed the width)."""
    assert t.ndim == 2
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    if t.shape[0] == 1 and t.stride(1) == 1:
        # a single row may carry any row stride (0 after numpy's [None]) and still count as contiguous
        return t.as_strided(t.shape, (t.shape[1], 1))
    return t.contiguous()


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def ss_output_length(Tx: int, F: int, hop: int) -> int:
    return min(Tx, (F - 1) * hop + 1)


# (ring width, largest order it serves) of the sample-wise filter's ring kernels (csrc/lpc_ss_plan.h GOLF_SS_TABLE): the time-chunked
# scan and the batch-parallel serial recursion need one ring width that divides the hop and exceeds the order.  Every other
# shape runs -- and trains -- on the wave-per-utterance kernels of csrc/lpc_any.hip.
SS_RINGS = ((8, 6), (16, 14), (24, 22), (32, 30), (40, 38))


def ss_is_trainable(M: int, hop: int, F: int = 2) -> bool:
    """True when (lpc order, hop) has a ring kernel.  Other shapes run forward and backward on the wave-per-utterance
    kernels (one serial recursion per utterance: ss_has_backward)."""
    return F >= 2 and any(M <= order and hop % ring == 0 for ring, order in SS_RINGS)


def ss_has_backward(M: int, hop: int, F: int = 2) -> bool:
    """True when ltv_allpole_ss differentiates at (lpc order, hop, frames): every 1 <= M <= 64, hop >= 1, F >= 1."""
    return 1 <= M <= 64 and hop >= 1 and F >= 1


def ss_has_f64(M: int, hop: int, F: int = 2) -> bool:
    """True when ltv_allpole_ss runs -- and differentiates -- (lpc order, hop, frames) in float64 (double tensors, or
    ``mode="fp64"``): every shape the fp32 filter serves, on or off the ring grid."""
    return ss_has_backward(M, hop, F)


# ------------------------------------------------------------------------------------------------
class _LTVAllPoleSS(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, gain, a, hop, prepared, fast_inference, mode=0, status=None, length=None):
        _lib.require_device(ex, gain, a)
        lib = _lib.load()
        ex = _rows(ex)
        gain = gain.contiguous()
        a = a.contiguous()
        B, Tx = ex.shape
        F, M = a.shape[1], a.shape[2]
        assert gain.shape == (B, F) and a.shape[0] == B
        T = ss_output_length(Tx, F, hop)
        if length is not None:   # only the first `length` samples of the excitation rows (no slice op on the caller's side)
            T = min(T, int(length))
            if T < 1:
                raise _lib.GolfError(f"ltv_allpole_ss: length={length} leaves nothing to filter")
        y = torch.empty(B, T, dtype=torch.float32, device=ex.device)
        side, flags = None, 0
        needs_grad = any(ctx.needs_input_grad[:3])
        if (prepared is not None and prepared.key == (B, T, F, M, hop, a.data_ptr(), a._version, mode)
                and not (prepared.fast and needs_grad and not prepared.training)):
            # (a caller with batches in flight keeps the thin pair of chunk passes with prepared maps too: without the flag the
            #  forward would take the one-launch form meant for a lone batch -- 50 vs 43 us/step measured, round 5)
            ws, flags, side = prepared.ws, HAVE_TRANSITIONS | mode | (THROUGHPUT if THROUGHPUT_MODE else 0), prepared.stream
            if prepared.fast:
                flags |= FAST_TRANSITIONS | (TRAINING if prepared.training else 0) | (MAPS_ONLY if prepared.maps_only else 0)
        else:
            if (THROUGHPUT_MODE and mode == 0 and not needs_grad and B >= SS_THROUGHPUT_SERIAL_MIN
                    and ex.stride(0) < SS_SERIAL_MAX_STRIDE):
                # several batches in flight: the plan that costs the least CHIP time (see the constant).  An explicit GOLF_SS_SERIAL
                # turns the library's quiet fallback for huge row strides into GOLF_EUNSUPPORTED, hence the stride test here (the
                # output is allocated dense above) -- a caller who asked for "auto" never sees that error.
                mode = SS_MODES["serial"]
            ws = _workspace(lib.golf_ltv_allpole_workspace_bytes_ex(B, T, F, M, hop, mode), ex.device)
            flags = mode | (THROUGHPUT if THROUGHPUT_MODE else 0)
            if fast_inference:
                # fp32 transition matrices (hot chunks recomputed from fp64 trajectories) + one refinement sweep; with a
                # gradient pending the forward also keeps the adjoint-orientation maps for the backward's own sweep
                flags |= FAST_TRANSITIONS | (TRAINING if needs_grad else 0)
            if SPLIT_P1:
                flags |= 4                # GOLF_SS_SPLIT_P1 (diagnostic): two launches instead of the fused one
            if FORK_TRANSITIONS:
                # the transition kernel (needs only `a`) and the zero-state pass (needs `ex`) are independent: the
                # library forks the former onto a side stream and joins before the boundary scan
                side = _side_stream(ex.device)
                ws.record_stream(side)
        rc = lib.golf_ltv_allpole_fwd_f32(ex.data_ptr(), ex.stride(0), gain.data_ptr(), a.data_ptr(), y.data_ptr(),
                                          y.stride(0), B, T, F, M, hop, ws.data_ptr(), ws.numel(), flags,
                                          side.cuda_stream if side is not None else 0, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_allpole_fwd_f32")
        if status is not None:
            # conditioning / health words of this forward (include/golf_amd.h golf_ltv_allpole_status_u32): written
            # asynchronously on the stream into the caller's 4-word device tensor, read by the host when it likes
            if not (status.is_cuda and status.numel() >= 4 and status.element_size() == 4 and status.is_contiguous()):
                raise _lib.GolfError("ltv_allpole_ss: `status` must be a contiguous device tensor of >= 4 32-bit words")
            rc = lib.golf_ltv_allpole_status_u32(ws.data_ptr(), ws.numel(), B, T, F, M, hop, flags, status.data_ptr(),
                                                 _lib.stream_ptr())
            _lib.check(rc, "golf_ltv_allpole_status_u32")
        ctx.hop, ctx.mode = hop, mode
        ctx.save_for_backward(ex, gain, a, y, ws)
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        ex, gain, a, y, ws = ctx.saved_tensors
        lib = _lib.load()
        hop = ctx.hop
        B, Tx = ex.shape
        F, M = a.shape[1], a.shape[2]
        T = y.shape[1]
        gy = _rows(gy.float())
        # the kernels write columns [0, T); the excitation's tail beyond the output length needs zeros: GOLF_SS_ZERO_TAIL has
        # the backward write them (a full-size fill was a 6 MB memset in front of every backward, a strided fill of the
        # tail alone still a launch: ~5 us of the B = 32 training step either way)
        g_ex = torch.empty(B, Tx, dtype=torch.float32, device=ex.device)
        g_gain = torch.empty_like(gain)
        g_a = torch.empty_like(a)
        rc = lib.golf_ltv_allpole_bwd_f32(gy.data_ptr(), gy.stride(0), y.data_ptr(), y.stride(0), ex.data_ptr(),
                                          ex.stride(0), gain.data_ptr(), a.data_ptr(), g_ex.data_ptr(),
                                          g_ex.stride(0), g_gain.data_ptr(), g_a.data_ptr(), B, T, F, M, hop,
                                          ws.data_ptr(), ws.numel(), ctx.mode | (ZERO_TAIL if Tx > T else 0),
                                          _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_allpole_bwd_f32")
        return g_ex, g_gain, g_a, None, None, None, None, None, None


class _LTVAllPoleF64(torch.autograd.Function):
    """The sample-wise filter with its recursion in float64 (golf_ltv_allpole_{fwd,bwd}_f64, csrc/lpc_any.hip): returns
    ``(y, state)``.  ``io`` = 1: float64 tensors in and out; 0: fp32 tensors, rounded once at the store.  ``zi`` (B, M) or None
    enters through the kernel's carried-state prologue; it may be a float64 tensor with fp32 I/O -- the ``state`` output of
    the block before, (B, M) float64 and NOT rounded to the I/O type, which is what keeps a chain of fp32 blocks on the bits
    of the one-shot call (ltv_allpole_ss_blocks).  ``state`` is None unless ``want_state``; it is differentiable."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, gain, a, zi, hop, length, io, want_state):
        dtype = torch.float64 if io else torch.float32
        _lib.require_device(ex, gain, a, dtype=dtype)
        if zi is not None:
            _lib.require_device(zi, dtype=dtype if zi.dtype == dtype else torch.float64)
        lib = _lib.load()
        ex = _rows(ex)
        gain = gain.contiguous()
        a = a.contiguous()
        B, Tx = ex.shape
        F, M = a.shape[1], a.shape[2]
        assert gain.shape == (B, F) and a.shape[0] == B and (zi is None or zi.shape == (B, M))
        T = ss_output_length(Tx, F, hop)
        if length is not None:
            T = min(T, int(length))
            if T < 1:
                raise _lib.GolfError(f"ltv_allpole_ss: length={length} leaves nothing to filter")
        y = torch.empty(B, T, dtype=dtype, device=ex.device)
        # the kernel's state buffer, in and out: the initial state on entry (zeros when only the final one is wanted)
        zi64 = None if zi is None else zi.to(torch.float64).contiguous()
        state = None
        if zi is not None or want_state:
            state = torch.zeros(B, M, dtype=torch.float64, device=ex.device) if zi is None else zi64.clone()
        rc = lib.golf_ltv_allpole_fwd_f64(ex.data_ptr(), ex.stride(0), gain.data_ptr(), a.data_ptr(), y.data_ptr(),
                                          y.stride(0), B, T, F, M, hop, _lib.ptr(state), io, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_allpole_fwd_f64")
        ctx.hop, ctx.io, ctx.zi_dtype = hop, io, None if zi is None else zi.dtype
        ctx.save_for_backward(ex, gain, a, y, zi64)
        ctx.set_materialize_grads(False)   # the cotangent of an unused state arrives as None
        return y, (state if want_state else None)

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy, g_state):
        ex, gain, a, y, zi64 = ctx.saved_tensors
        lib = _lib.load()
        hop, io = ctx.hop, ctx.io
        B, Tx = ex.shape
        F, M = a.shape[1], a.shape[2]
        T = y.shape[1]
        want_ex, want_gain, want_a, want_zi = ctx.needs_input_grad[:4]
        if gy is None and g_state is None:
            return (None,) * 8
        gy = torch.zeros_like(y) if gy is None else gy.to(y.dtype)
        H = min(M, T)
        if g_state is not None:   # state[:, j] = y[:, T-1-j] (j < T), zi[:, j-T] beyond: its cotangent joins theirs
            gy = gy.clone()
            gy[:, T - H:] += g_state[:, :H].flip(1).to(y.dtype)
        gy = _rows(gy)
        g_ex = torch.empty(B, Tx, dtype=y.dtype, device=ex.device) if want_ex else None   # (the tail's zeros: the kernel)
        g_gain = torch.empty_like(gain) if want_gain else None
        g_a = torch.empty_like(a) if want_a else None
        g_zi = torch.empty(B, M, dtype=torch.float64, device=ex.device) if want_zi else None
        ws = _workspace(lib.golf_ltv_allpole_f64_workspace_bytes(B, T), ex.device)
        rc = lib.golf_ltv_allpole_bwd_f64(gy.data_ptr(), gy.stride(0), y.data_ptr(), y.stride(0), ex.data_ptr(), ex.stride(0),
                                          gain.data_ptr(), a.data_ptr(), _lib.ptr(zi64), _lib.ptr(g_ex), Tx, Tx,
                                          _lib.ptr(g_gain), _lib.ptr(g_a), _lib.ptr(g_zi), B, T, F, M, hop, ws.data_ptr(),
                                          ws.numel(), io, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_allpole_bwd_f64")
        if g_zi is not None:
            if g_state is not None and T < M:
                g_zi[:, :M - T] += g_state[:, T:]
            g_zi = g_zi.to(ctx.zi_dtype)
        return g_ex, g_gain, g_a, g_zi, None, None, None, None


def _ss_route(ex, gain, a, zi, mode, status=None):
    """The checks of ``zi`` and ``status`` and the choice of _ss_f64_io, for ltv_allpole_ss and ltv_allpole_ss_blocks."""
    if zi is not None and (zi.dim() != 2 or a.dim() != 3 or tuple(zi.shape) != (a.shape[0], a.shape[2])):
        raise _lib.GolfError(f"ltv_allpole_ss: zi {tuple(zi.shape)} for a {tuple(a.shape)}: a (B, M) initial state required")
    io = _ss_f64_io(ex, gain, a, zi, mode)
    if zi is not None and (zi.device != ex.device or not zi.is_floating_point()
                           or (zi.dtype not in (torch.float32, torch.float64) and not torch.is_autocast_enabled())):
        raise _lib.GolfError(f"ltv_allpole_ss: zi must be an fp32 (or, with float64 tensors, a float64) tensor on {ex.device} "
                             f"(got {zi.dtype} on {zi.device})")
    if io is not None and status is not None:
        raise _lib.GolfError("ltv_allpole_ss: `status` does not apply to the float64 recursion (double tensors, mode=\"fp64\"): "
                             "the status words describe the conditioning tiers of the time-chunked fp32 scan")
    return io


def _ss_f64_io(ex, gain, a, zi, mode):
    """Which kernels serve a call of ltv_allpole_ss: None -- the fp32 ones; 1 -- the float64 recursion on float64 tensors;
    0 -- the same recursion on fp32 tensors (``mode="fp64"``).  Tensors of different dtypes raise, whatever their device.
    Under autocast every input is cast to fp32 as ever (float64 ones are left alone by torch.amp and refused as before)."""
    if torch.is_autocast_enabled():
        return 0 if mode == "fp64" else None
    named = [(n, t) for n, t in (("ex", ex), ("gain", gain), ("a", a), ("zi", zi)) if t is not None]
    if len({t.dtype for _, t in named}) > 1:
        raise _lib.GolfError("ltv_allpole_ss: " + ", ".join(f"{n} is {t.dtype}" for n, t in named)
                             + ": one dtype required (all fp32, or all float64 for the float64 recursion)")
    if ex.dtype == torch.float64:
        return 1
    return 0 if mode == "fp64" else None


class _LTVAllPoleHead(torch.autograd.Function):
    """xh = ex*up(gain) - c, c the part of the first min(M, T) samples' recursion that reads the initial state ``zi`` (B, M)
    (golf_ltv_allpole_head_{fwd,bwd}_f32): the zero-state filter of xh with gain == 1 IS the filter of ex from zi."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, gain, a, zi, hop, T):
        _lib.require_device(ex, gain, a, zi)
        lib = _lib.load()
        ex = _rows(ex)
        gain, a, zi = gain.contiguous(), a.contiguous(), zi.contiguous()
        B, F, M = a.shape
        assert ex.shape[0] == B and gain.shape == (B, F) and zi.shape == (B, M) and 1 <= T <= ex.shape[1]
        xh = torch.empty(B, T, dtype=torch.float32, device=ex.device)
        rc = lib.golf_ltv_allpole_head_fwd_f32(ex.data_ptr(), ex.stride(0), gain.data_ptr(), a.data_ptr(), zi.data_ptr(),
                                               xh.data_ptr(), xh.stride(0), B, T, F, M, hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_allpole_head_fwd_f32")
        ctx.hop = hop
        ctx.save_for_backward(ex, gain, a, zi)
        return xh

    @staticmethod
    @_amp_bwd
    def backward(ctx, q):
        ex, gain, a, zi = ctx.saved_tensors
        lib = _lib.load()
        B, Tx = ex.shape
        F, M = a.shape[1], a.shape[2]
        q = _rows(q.float())
        T = q.shape[1]
        want_ex, want_gain, want_a, want_zi = ctx.needs_input_grad[:4]
        g_ex = torch.empty(B, Tx, dtype=torch.float32, device=ex.device) if want_ex else None
        g_gain = torch.empty_like(gain) if want_gain else None
        g_a = torch.empty_like(a) if want_a else None
        g_zi = torch.empty_like(zi) if want_zi else None
        rc = lib.golf_ltv_allpole_head_bwd_f32(q.data_ptr(), q.stride(0), ex.data_ptr(), ex.stride(0), gain.data_ptr(),
                                               a.data_ptr(), zi.data_ptr(), _lib.ptr(g_ex), Tx, Tx, _lib.ptr(g_gain),
                                               _lib.ptr(g_a), _lib.ptr(g_zi), B, T, F, M, ctx.hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_allpole_head_bwd_f32")
        return g_ex, g_gain, g_a, g_zi, None, None


SS_MODES = {None: 0, "auto": 0, "serial": 8, "chunked": 16, "flat-scan": 16 | 32}   # GOLF_SS_SERIAL / _CHUNKED / _FLAT_SCAN
# Set by a caller that keeps several batches in flight (bench.py's pipelined loop, a serving loop): GOLF_SS_THROUGHPUT
# is added to every sample-wise filter call.  Bit-identical results WITHIN one algorithm (the flag only changes the launch
# chain of the time-chunked scan); from SS_THROUGHPUT_SERIAL_MIN utterances on this module additionally switches an inference
# forward to the serial kernels, which are another algorithm: same accuracy class, different bits (and a forward through a
# PreparedTransitions handle keeps the chunked scan its maps were made for).  A lone batch takes ~10 us longer, four in
# flight finish ~2 % more per second (include/golf_amd.h).
THROUGHPUT_MODE = False
# With batches in flight (THROUGHPUT_MODE) an inference forward of this many utterances or more takes the batch-parallel
# serial kernels instead of the time-chunked scan (the library's own switch, for a lone batch, is at 2048).  The chunked
# scan does ~12 x the sequential arithmetic to finish ONE batch soon and saturates the chip at ~29 G samples/s whatever the
# batch; the serial kernels do 1 x, take ~2.4 ms per batch whatever its size, and leave the chip to the other batches.
# Whole synthesis step, MI355X, G samples/s (round 5): B = 256 chunked 28.8 | serial x 8 streams 24.5;  B = 1024 chunked 29.0 |
# serial x 4 streams 42.6, x 8 streams 57.4;  B = 2048 (serial either way) x 1 stream 29.0, x 4 streams 57.4.
SS_THROUGHPUT_SERIAL_MIN = 512
SS_SERIAL_MAX_STRIDE = 1 << 24   # the serial kernels address 16 rows through one 32-bit buffer descriptor (lpc_ss.hip serial_strides_ok)


def ltv_allpole_ss(ex: torch.Tensor, gain: torch.Tensor, a: torch.Tensor, hop: int,
                   prepared: "PreparedTransitions" = None, fast_inference: bool = True,
                   mode: str = None, status: torch.Tensor = None, length: int = None,
                   zi: torch.Tensor = None, return_zf: bool = False):
    """y[t] = ex[t]*up(gain)[t] - sum_i up(a)[t,i] y[t-1-i]; ex (B,Tx), gain (B,F), a (B,F,M) at hop.
    Output (B, min(Tx,(F-1)*hop+1)).  Differentiable w.r.t. ex, gain, a (custom HIP backward).
    Float64: with ``ex``, ``gain``, ``a`` (and ``zi``) all float64 the recursion, its adjoint and the gradient sums run in
    double on the device (csrc/lpc_any.hip: one wave per utterance, every shape with 1 <= M <= 64) and the result and the
    gradients are float64 -- what torchlpc.sample_wise_lpc computes for double inputs, and what torch.autograd.gradcheck
    can be pointed at.  ``prepared``, ``fast_inference`` and any ``mode`` are ignored then; ``status`` raises (its words
    describe the chunked scan); ``length``, ``zi`` and ``return_zf`` work as in fp32.  Tensors of different dtypes raise.
    ``prepared``: handle from ltv_allpole_prepare(a, hop, T) (ignored if it does not match).
    ``fast_inference``: when no input requires grad, use fp32 transition matrices + one refinement sweep instead of
    fp64 matrices (same accuracy class as a sequential fp32 recursion, ~4x less work in the dominant kernel).
    ``mode``: "fp64" runs fp32 tensors through the float64 recursion -- fp32 in and out, every value widened at the load and
    rounded once at the store: for the utterances at the edge of stability, where no fp32 recursion reaches 1e-4 (rows that
    ``status`` counts as hot), at the cost of one serial recursion per utterance.  With float64 tensors
    it is the same as no mode.  Otherwise None/"auto" picks the algorithm by batch size (time-chunked scan below 2048 utterances, batch-parallel
    serial recursion from there on: include/golf_amd.h GOLF_SS_SERIAL); "serial" / "chunked" force one.  "flat-scan"
    forces the chunked algorithm's flat boundary scan.  That is not only a diagnostic: "auto" itself takes the flat scan for
    every lone batch of more than ~40 utterances below the serial threshold (lpc_ss_plan.h ss_two_level; the two-level scan
    is the faster form only while B x groups <= 2 x the CU count) and whenever an utterance has fewer than 48 chunk maps.  Both
    scans are held to the same bound -- 3 e_sequential_fp32 + 1e-4 of the float64 oracle forward, + 2e-4 for the gradients -- by
    the suite's soak (tests/test_gpu_lpc_ss.py::test_conditioning_soak_bounded, ::test_round5_soak_exceedances) and by
    tools/fuzz_tiers.py over eleven seeds x 120 cases (round 6: no row beyond it on either scan).
    ``length``: filter only the first ``length`` samples of ``ex`` (output (B, min(length, natural length))): what
    ``ltv_allpole_ss(ex[:, :length], ...)`` computes, without the slice -- whose backward would be a full-size fill and a
    full-size copy in front of the producer's backward (the gradient of the unused tail is written as zeros by the filter's
    own backward, GOLF_SS_ZERO_TAIL).
    ``status``: optional int32 device tensor of >= 4 elements that receives, asynchronously, the conditioning / health
    words of this call (decode with ss_status): utterances with recomputed chunk maps, utterances on the fp64 boundary
    scan, non-finite output flag, largest transition-matrix entry.
    ``zi``: initial state (B, M) fp32, y[b, -1-j] = zi[b, j] (torchlpc.sample_wise_lpc's ``zi``); None = zeros, and then the
    call is exactly the one without the argument: same launches, same bits.  With ``zi`` the state enters as a correction of
    the first min(M, T) excitation samples (golf_ltv_allpole_head_fwd_f32) in front of the same filter, so every plan and every
    ``mode`` serves it, and the result is differentiable w.r.t. ``zi`` as well.
    ``return_zf``: return ``(y, zf)`` with zf (B, M) the final state, zf[b, j] = y[b, T-1-j] (for T < M the initial state
    shifted in behind the T outputs): the ``zi`` of the block that follows.  It stays in the graph, so a chain of blocks is
    differentiable through the state (ltv_allpole_ss_blocks)."""
    io = _ss_route(ex, gain, a, zi, mode, status)
    if ex.dim() == 2 and (ex.shape[0] == 0 or ex.shape[1] == 0):
        # an empty batch / zero samples: what the reference's tensor ops return (an empty result that stays in the graph);
        # the C ABI itself rejects non-positive sizes
        _lib.require_device(ex, gain, a, dtype=torch.float64 if io == 1 else torch.float32)
        T = ss_output_length(ex.shape[1], a.shape[1], int(hop)) if ex.shape[1] else 0
        if length is not None:
            T = min(T, max(int(length), 0))
        y = ex[:, :T] * 1.0 + 0.0 * (gain.sum() + a.sum())
        return (y, _final_state(y, zi, a.shape[2])) if return_zf else y
    if io is not None:
        # the state enters through the kernel's prologue; zf below is read off y (and zi) like the fp32 path's
        y = _LTVAllPoleF64.apply(ex, gain, a, zi, int(hop), length, io, False)[0]
    elif zi is None:
        y = _LTVAllPoleSS.apply(ex, gain, a, int(hop), prepared, bool(fast_inference), SS_MODES[mode], status, length)
    else:
        T = ss_output_length(ex.shape[1], a.shape[1], int(hop))
        if length is not None:
            T = min(T, int(length))
            if T < 1:
                raise _lib.GolfError(f"ltv_allpole_ss: length={length} leaves nothing to filter")
        xh = _LTVAllPoleHead.apply(ex, gain, a, zi, int(hop), T)
        # (the maps of `prepared`, the mode and the status words depend on `a` alone: they pass through)
        y = _LTVAllPoleSS.apply(xh, torch.ones_like(gain, dtype=torch.float32), a, int(hop), prepared, bool(fast_inference),
                                SS_MODES[mode], status, length)
    return (y, _final_state(y, zi, a.shape[2])) if return_zf else y


def _final_state(y: torch.Tensor, zi, M: int) -> torch.Tensor:
    """zf (B, M): zf[:, j] = y[:, T-1-j] for j < T, the initial state shifted by T behind them.  Plain indexing: autograd adds
    the cotangent of zf into y's (and zi's) by itself."""
    T = y.shape[1]
    if T >= M:
        return y[:, T - M:].flip(1)
    old = zi[:, :M - T].to(y.dtype) if zi is not None else y.new_zeros(y.shape[0], M - T)
    return torch.cat([y.flip(1), old], 1)


def ltv_allpole_ss_blocks(ex: torch.Tensor, gain: torch.Tensor, a: torch.Tensor, hop: int, frames_per_block: int,
                          zi: torch.Tensor = None, detach_state: bool = False, length: int = None, **kw):
    """ltv_allpole_ss over blocks of ``frames_per_block`` frames chained through the state: returns ``(y, zf)``, y what the
    one-shot call returns (up to fp32 rounding: a block's plan sees another utterance length) and zf (B, M) the final state.
    Block k filters the samples [k*n*hop, (k+1)*n*hop), n = frames_per_block, with the frames k*n .. (k+1)*n (a block needs
    the frame that ends it for the interpolation); the last block ends with the utterance, sample (F-1)*hop included.
    ``detach_state=True`` cuts the gradient at every block boundary (truncated back-propagation through time): same y.
    ``zi``: the state in front of the first block.  ``**kw``: fast_inference / mode / status of ltv_allpole_ss.
    With float64 tensors, or ``mode="fp64"``, the blocks run the float64 recursion and hand each other its state in double --
    with fp32 tensors too, where zf alone is rounded: y and zf are then the BITS of the one-shot call, wherever the blocks end."""
    hop, n = int(hop), int(frames_per_block)
    if n < 1:
        raise _lib.GolfError(f"ltv_allpole_ss_blocks: frames_per_block={frames_per_block} must be >= 1")
    if "prepared" in kw or "return_zf" in kw:
        raise _lib.GolfError("ltv_allpole_ss_blocks: `prepared` / `return_zf` do not apply to a chain of blocks")
    F = a.shape[1]
    T = ss_output_length(ex.shape[1], F, hop)
    if length is not None:
        T = min(T, max(int(length), 0))
    if ex.shape[0] == 0 or T == 0:
        return ltv_allpole_ss(ex, gain, a, hop, length=length, zi=zi, return_zf=True, **kw)
    parts, state = [], zi
    if _ss_route(ex, gain, a, zi, kw.get("mode"), kw.get("status")) == 0:
        # fp32 tensors through the float64 recursion: zf as ltv_allpole_ss returns it is rounded to fp32, the kernel's own
        # state is not (float64 tensors need nothing of the kind: their zf IS the state, and they take the loop below)
        for f0, f1, t0, t1 in ss_block_bounds(T, F, hop, n):
            y, state = _LTVAllPoleF64.apply(ex[:, t0:t1], gain[:, f0:f1 + 1], a[:, f0:f1 + 1], state, hop, None, 0, True)
            parts.append(y)
            if detach_state:
                state = state.detach()
        return (parts[0] if len(parts) == 1 else torch.cat(parts, 1)), state.to(parts[0].dtype)
    for f0, f1, t0, t1 in ss_block_bounds(T, F, hop, n):
        y, state = ltv_allpole_ss(ex[:, t0:t1], gain[:, f0:f1 + 1], a[:, f0:f1 + 1], hop, zi=state, return_zf=True, **kw)
        parts.append(y)
        if detach_state:
            state = state.detach()
    return (parts[0] if len(parts) == 1 else torch.cat(parts, 1)), state


def ss_block_bounds(T: int, F: int, hop: int, frames_per_block: int):
    """[(f0, f1, t0, t1)] of ltv_allpole_ss_blocks: block k takes the frames f0 .. f1 inclusive and the samples [t0, t1) of an
    utterance of T <= (F-1)*hop+1 output samples.  Blocks start on frame boundaries; only the last one holds the sample that
    ends its last frame; frames past the T-th sample get no block."""
    if F == 1:
        return [(0, 0, 0, min(T, 1))]
    out = []
    for f0 in range(0, F - 1, frames_per_block):
        f1 = min(f0 + frames_per_block, F - 1)
        t0, t1 = f0 * hop, min(f1 * hop + (1 if f1 == F - 1 else 0), T)
        if t0 >= T:
            break
        out.append((f0, f1, t0, t1))
    return out


def _inference_only(what: str, *tensors) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(f"golf_amd: {what} is inference only (an input requires grad)")


def ltv_allpole_ss_state(ex: torch.Tensor, gain: torch.Tensor, a: torch.Tensor, hop: int, state: torch.Tensor,
                         mode: str = "serial") -> torch.Tensor:
    """ltv_allpole_ss from a carried state (golf_ltv_allpole_fwd_state_f32): y[b, -1-i] = state[b, i],
    output (B, min(Tx, (F-1)*hop+1)); ``state`` (B, M) fp32 is updated in place to the block's last M outputs.  Inference only.
    ``mode="serial"`` (the default) is always the serial recursion: blocks that start on frame boundaries, chained through
    ``state`` from zeros, give the bits of ``ltv_allpole_ss(..., mode="serial")`` over the whole.  Any other ``mode`` of
    ltv_allpole_ss (None / "auto", "chunked", "flat-scan") runs ``ltv_allpole_ss(zi=state, return_zf=True)`` on that plan --
    the fast ones for long blocks -- and copies the final state into ``state``: the same accuracy class, but ONLY "serial"
    gives bits that do not depend on where the blocks are cut.  For a state that carries gradients call ltv_allpole_ss(zi=...)
    itself."""
    _inference_only("ltv_allpole_ss_state", ex, gain, a)
    if mode != "serial":
        if tuple(state.shape) != (a.shape[0], a.shape[2]) or not state.is_contiguous():
            raise _lib.GolfError(f"ltv_allpole_ss_state: a {tuple(a.shape)}, state {tuple(state.shape)} "
                                 "(contiguous (B, M) required)")
        with torch.no_grad():
            y, zf = ltv_allpole_ss(ex, gain, a, hop, mode=mode, zi=state, return_zf=True)
            state.copy_(zf)
        return y
    ex, gain, a = _rows(ex.float()), gain.float().contiguous(), a.float().contiguous()   # (autocast: fp16/bf16 tracks first)
    _lib.require_device(ex, gain, a, state)
    B, Tx = ex.shape
    F, M = a.shape[1], a.shape[2]
    if gain.shape != (B, F) or a.shape[0] != B or state.shape != (B, M) or not state.is_contiguous():
        raise _lib.GolfError(f"ltv_allpole_ss_state: ex {tuple(ex.shape)}, gain {tuple(gain.shape)}, a {tuple(a.shape)}, "
                             f"state {tuple(state.shape)} (contiguous (B, M) required)")
    T = ss_output_length(Tx, F, int(hop))
    y = torch.empty(B, T, dtype=torch.float32, device=ex.device)
    lib = _lib.load()
    rc = lib.golf_ltv_allpole_fwd_state_f32(ex.data_ptr(), ex.stride(0), gain.data_ptr(), a.data_ptr(), y.data_ptr(),
                                            y.stride(0), B, T, F, M, int(hop), state.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "golf_ltv_allpole_fwd_state_f32")
    return y


def ss_status(status: torch.Tensor, warn: bool = True) -> dict:
    """Decode the 4 status words of ltv_allpole_ss(..., status=t) (synchronises: reads the device tensor).  ``warn=False``:
    the caller reports a fix-up timeout itself (the module's health monitor: one warning per event, not two)."""
    w = status.detach().to("cpu").view(torch.int32)[:4]
    if warn and int(w[2]) & 2:   # never observed; a wait that ran out means the maps of a hot utterance may be half-updated
        import warnings

        warnings.warn("golf_amd: a device-side wait for the chunk-map fix-up ran out (golf_ltv_allpole_status_u32 bit 1): "
                      "the output of hot utterances of this forward is not trustworthy", RuntimeWarning)
    return {"hot_utterances": int(w[0]), "tier3_utterances": int(w[1]), "nonfinite": bool(int(w[2]) & 1),
            "fixup_timeout": bool(int(w[2]) & 2), "scan_mismatch": bool(int(w[2]) & 4),
            "max_phi": float(w[3:4].view(torch.float32)[0])}


class _LTVInverse(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, y, a, hop):
        _lib.require_device(y, a)
        lib = _lib.load()
        y = _rows(y)
        a = a.contiguous()
        B, Ty = y.shape
        F, M = a.shape[1], a.shape[2]
        T = ss_output_length(Ty, F, hop)
        e = torch.empty(B, T, dtype=torch.float32, device=y.device)
        rc = lib.golf_ltv_inverse_f32(y.data_ptr(), y.stride(0), a.data_ptr(), e.data_ptr(), e.stride(0), B, T, F, M,
                                      hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_inverse_f32")
        ctx.save_for_backward(y, a)
        ctx.geom = (hop, T)
        return e

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_e):
        y, a = ctx.saved_tensors
        hop, T = ctx.geom
        lib = _lib.load()
        g_e = _rows(g_e)
        B, Ty = y.shape
        F, M = a.shape[1], a.shape[2]
        need_y, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_y = (torch.empty_like(y) if Ty == T else torch.zeros_like(y)) if need_y else None
        g_a = torch.empty_like(a) if need_a else None
        rc = lib.golf_ltv_inverse_bwd_f32(g_e.data_ptr(), g_e.stride(0), y.data_ptr(), y.stride(0), a.data_ptr(),
                                          g_y.data_ptr() if need_y else None, g_y.stride(0) if need_y else 0,
                                          g_a.data_ptr() if need_a else None, B, T, F, M, hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_inverse_bwd_f32")
        return g_y, g_a, None


def ltv_inverse(y: torch.Tensor, a: torch.Tensor, hop: int) -> torch.Tensor:
    """e[t] = y[t] + sum_i up(a)[t,i] y[t-1-i] (analysis filter); differentiable w.r.t. y and a."""
    return _LTVInverse.apply(y, a, hop)


RES_MAX_ORDER = 64   # csrc/lpc_residual.hip RES_MAX_M


def _analysis_head(who, x, c, name, hop, sample_rate=None, a=None) -> int:
    """What the analyses of x (B, T) beside a frame-rate track ``c`` (B, F), named ``name``, refuse first: the shapes (with
    those of ``a`` (B, F, M) where there is one), ``hop < 1`` and a sample rate that is not positive.  Returns the hop."""
    if x.dim() != 2:
        raise _lib.GolfError(f"{who}: x must be (B, T) (got {tuple(x.shape)})")
    if c.dim() != 2 or c.shape[0] != x.shape[0]:
        raise _lib.GolfError(f"{who}: {name} must be (B, F) with the B of x (got {tuple(c.shape)}, x {tuple(x.shape)})")
    if a is not None and (a.dim() != 3 or a.shape[:2] != c.shape):
        raise _lib.GolfError(f"{who}: a must be (B, F, M) with the (B, F) of {name} (got {tuple(a.shape)}, {name} "
                             f"{tuple(c.shape)})")
    hop = int(hop)
    if hop < 1:
        raise _lib.GolfError(f"{who}: hop={hop} must be >= 1")
    if sample_rate is not None and not sample_rate > 0:
        raise _lib.GolfError(f"{who}: sample_rate={sample_rate} must be positive")
    return hop


def _check_frames(who, name, n, least, B=None) -> None:
    """The frame count ``name`` = n is at least ``least`` and, with ``B``, small enough for the library (which refuses it too;
    here before the outputs are allocated)."""
    if n < least:
        raise _lib.GolfError(f"{who}: {name}={n} frames, must be >= {least}")
    if B is not None and B * n >= 2 ** 31:
        raise _lib.GolfError(f"{who}: B*{name} = {B * n} frames, must be < 2^31")


def _check_far(who, hop, first, v, count, n, a, va, b, vb) -> None:
    """The positions of a stream entry stay where ``position * hop`` cannot overflow: the two named ``a`` and ``b`` in
    0..2^62, and the frames from the one named ``first`` with the ``count`` = n after them below 2^62 / hop."""
    far = 2 ** 62
    for name, value in ((a, va), (b, vb)):
        if not 0 <= value <= far:
            raise _lib.GolfError(f"{who}: {name}={value} must be 0..2^62")
    if not 0 <= v <= far // hop - n:
        raise _lib.GolfError(f"{who}: {first}={v} must be >= 0 with ({first} + {count}) hop <= 2^62")


@_amp_no_grad   # an analysis without a backward (ltv_inverse has one): inference only, like harmonic_analysis
def _ltv_residual(x, gain, a, pos, n_out, hop):
    """``pos``: None for the one-shot entry, ``(x_t0, fr_first, t_first, last)`` for the stream entry."""
    _lib.require_device(x, gain, a)
    lib = _lib.load()
    x, gain, a = _rows(x), gain.contiguous(), a.contiguous()
    B, M = x.shape[0], a.shape[2]
    e = torch.empty(B, n_out, dtype=torch.float32, device=x.device)
    if pos is None:
        rc = lib.golf_ltv_residual_f32(x.data_ptr(), x.stride(0), gain.data_ptr(), a.data_ptr(), e.data_ptr(), e.stride(0), B,
                                       x.shape[1], a.shape[1], M, hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_residual_f32")
    else:
        x_t0, fr_first, t_first, last = pos
        rc = lib.golf_ltv_residual_stream_f32(x.data_ptr(), x.stride(0), x_t0, x.shape[1], gain.data_ptr(), a.data_ptr(),
                                              fr_first, a.shape[1], e.data_ptr(), e.stride(0), B, t_first, n_out, int(last),
                                              M, hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_residual_stream_f32")
    return e


def _residual_shapes(who, x, gain, a, hop):
    hop, M = _analysis_head(who, x, gain, "gain", hop, a=a), a.shape[2]
    if not 1 <= M <= RES_MAX_ORDER:
        raise _lib.GolfError(f"{who}: M={M} (the last dimension of a) must be 1..{RES_MAX_ORDER}")
    return hop, M


def _residual_empty(x, gain, a, n_out):
    _lib.require_device(x.float(), gain.float(), a.float())
    return torch.empty(x.shape[0], n_out, dtype=torch.float32, device=x.device)


def ltv_residual(x: torch.Tensor, gain: torch.Tensor, a: torch.Tensor, hop: int) -> torch.Tensor:
    """The decoder's excitation estimate in one launch (golf_ltv_residual_f32, the definition is in include/golf_amd.h):
    x (B, T), ``gain`` (B, F) and ``a`` (B, F, M) as ``lpc_analysis`` gives them -> ``e (B, T')``, ``T' = min(T, (F - 1) hop +
    1)``: ``ltv_inverse(x, a, hop)``, bit for bit, divided by the gain interpolated as ``fmaf(w, gain[f+1] - gain[f],
    gain[f])`` with ``w = (t - f hop) / hop``, one correctly rounded division each.  Every sample is a function of its
    position alone, which is what ``ltv_residual_stream`` is exact against; it differs from ``ltv_inverse(x, a, hop) /
    linear_upsample(gain, hop)`` only in how the gain is interpolated.  No gradient: the output never requires grad;
    strided rows of x are read in place.  An empty batch or an empty x returns an empty result without a launch."""
    who = "ltv_residual"
    hop, M = _residual_shapes(who, x, gain, a, hop)
    (B, T), F = x.shape, gain.shape[1]
    _check_frames(who, "F", F, 1)
    n_out = ss_output_length(T, F, hop)
    if B == 0 or n_out == 0:
        return _residual_empty(x, gain, a, n_out)
    return _ltv_residual(x, gain, a, None, n_out, hop)


def ltv_residual_stream(x: torch.Tensor, gain: torch.Tensor, a: torch.Tensor, x_t0: int, fr_first: int, t_first: int,
                        n_out: int, last: bool, hop: int) -> torch.Tensor:
    """``ltv_residual`` at a position of a longer utterance (golf_ltv_residual_stream_f32, include/golf_amd.h): samples
    ``t_first .. t_first + n_out - 1`` from x (B, n_x), the utterance's samples ``[x_t0, x_t0 + n_x)``, and ``gain`` (B, n_fr),
    ``a`` (B, n_fr, M), its frames ``[fr_first, fr_first + n_fr)``; ``last``: the utterance ends with these frames (F =
    ``fr_first + n_fr``).  Each sample has the bits the one-shot call gives it.  The buffers must hold what the samples read:
    ``0 <= x_t0 <= max(0, t_first - M)``, ``x_t0 + n_x >= t_first + n_out``, ``fr_first <=`` the frame of ``t_first`` and,
    unless ``last``, ``(t_first + n_out - 1) // hop + 1 < fr_first + n_fr``; with ``last``, ``t_first + n_out <= (F - 1) hop +
    1``; anything else raises ``GolfError`` before a launch.  ``n_out = 0`` or an empty batch returns an empty result without
    a launch."""
    who = "ltv_residual_stream"
    hop, M = _residual_shapes(who, x, gain, a, hop)
    x_t0, fr_first, t_first, n_out, last = int(x_t0), int(fr_first), int(t_first), int(n_out), bool(last)
    (B, n_x), n_fr = x.shape, gain.shape[1]
    if n_out < 0:
        raise _lib.GolfError(f"{who}: n_out={n_out} must be >= 0")
    _check_far(who, hop, "fr_first", fr_first, "n_fr", n_fr, "x_t0", x_t0, "t_first", t_first)
    if n_out:
        t_end, x_end, fr_end = t_first + n_out, x_t0 + n_x, fr_first + n_fr
        if n_fr < 1:
            raise _lib.GolfError(f"{who}: n_fr={n_fr} frames, must be >= 1")
        if x_t0 > max(t_first - M, 0):
            raise _lib.GolfError(f"{who}: x_t0={x_t0} lies above sample {max(t_first - M, 0)}, the first tap of sample "
                                 f"t_first={t_first}")
        if x_end < t_end:
            raise _lib.GolfError(f"{who}: x ends at sample {x_end} (n_x={n_x}), before the last computed sample {t_end - 1}")
        f_lo = t_first // hop
        if last:
            if t_end > (fr_end - 1) * hop + 1:
                raise _lib.GolfError(f"{who}: n_out={n_out}: the samples end at {t_end}, beyond (F - 1) hop + 1 = "
                                     f"{(fr_end - 1) * hop + 1} of the F={fr_end} frames the utterance ends with")
            f_lo = min(f_lo, max(fr_end - 2, 0))
        elif (t_end - 1) // hop + 1 >= fr_end:
            raise _lib.GolfError(f"{who}: the frames end at {fr_end} (n_fr={n_fr}), without frame {(t_end - 1) // hop + 1} "
                                 f"after the last sample {t_end - 1}, and last is not set")
        if fr_first > f_lo:
            raise _lib.GolfError(f"{who}: fr_first={fr_first} lies above frame {f_lo} of the first sample t_first={t_first}")
    if B == 0 or n_out == 0:
        return _residual_empty(x, gain, a, n_out)
    return _ltv_residual(x, gain, a, (x_t0, fr_first, t_first, last), n_out, hop)


# ------------------------------------------------------------------------------------------------
# LPC analysis: audio -> (gain, a, rc) per frame (include/golf_amd.h, csrc/lpc_analysis.hip)
# ------------------------------------------------------------------------------------------------
def lpc_analysis_frames(T: int, W: int, hop: int, centred: bool = True) -> int:
    """Frames of the analysis: ``T // hop + 1`` centred (the filters' frame grid and the center=True STFT count),
    ``max(T - W, 0) // hop + 1`` for frames that start at sample 0."""
    return T // hop + 1 if centred else max(T - W, 0) // hop + 1


class _LPCAnalysis(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, window, hop, M, origin, F, eps_rel, eps_abs, want_rc):
        _lib.require_device(x, window)
        lib = _lib.load()
        x = _rows(x)
        window = window.contiguous()
        B, T = x.shape
        W = window.numel()
        gain = torch.empty(B, F, dtype=torch.float32, device=x.device)
        a = torch.empty(B, F, M, dtype=torch.float32, device=x.device)
        rc = torch.empty(B, F, M, dtype=torch.float32, device=x.device) if want_rc else None   # not asked for: not written
        ws = _workspace(lib.golf_lpc_analysis_workspace_bytes(B, F, M), x.device)
        rcode = lib.golf_lpc_analysis_fwd_f32(x.data_ptr(), x.stride(0), window.data_ptr(), gain.data_ptr(), a.data_ptr(),
                                              _lib.ptr(rc), ws.data_ptr(), ws.numel(), B, T, F, M, hop, W, origin,
                                              eps_rel, eps_abs, _lib.stream_ptr())
        _lib.check(rcode, "golf_lpc_analysis_fwd_f32")
        ctx.save_for_backward(x, window, ws)   # ws holds the regularised lags in fp64: the backward starts from them
        ctx.geom = (hop, M, origin, F, eps_rel)
        ctx.set_materialize_grads(False)   # the gradient of an unused output arrives as None, not as a tensor of zeros
        return (gain, a, rc) if want_rc else (gain, a)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_gain, g_a, g_rc=None):
        x, window, lags = ctx.saved_tensors
        hop, M, origin, F, eps_rel = ctx.geom
        if not ctx.needs_input_grad[0] or (g_gain is None and g_a is None and g_rc is None):
            return (None,) * 9
        lib = _lib.load()
        B, T = x.shape
        # an output nobody differentiated arrives as None and goes to the kernel as a null pointer: it is never read
        gs = [None if g is None else g.float().contiguous() for g in (g_gain, g_a, g_rc)]
        g_x = torch.empty(B, T, dtype=torch.float32, device=x.device)   # written in full by the gather
        ws = _workspace(lib.golf_lpc_analysis_workspace_bytes(B, F, M), x.device)
        rcode = lib.golf_lpc_analysis_bwd_f32(_lib.ptr(gs[0]), _lib.ptr(gs[1]), _lib.ptr(gs[2]), x.data_ptr(), x.stride(0),
                                              window.data_ptr(), lags.data_ptr(), g_x.data_ptr(), g_x.stride(0),
                                              ws.data_ptr(), ws.numel(), B, T, F, M, hop, window.numel(), origin, eps_rel,
                                              _lib.stream_ptr())
        _lib.check(rcode, "golf_lpc_analysis_bwd_f32")
        return (g_x,) + (None,) * 8


def lpc_analysis(x: torch.Tensor, window: torch.Tensor, hop: int, order: int, centred: bool = True, n_frames: int = None,
                 eps_rel: float = 1e-9, eps_abs: float = 1e-12, return_rc: bool = False):
    """Frame-wise LPC analysis by the autocorrelation method: x (B, T), window (W,) -> ``(gain (B, F), a (B, F, order))`` or,
    with ``return_rc``, ``(gain, a, rc)``.  Frame f reads ``x[f*hop - W//2 + k] * window[k]`` (``centred``, F = T // hop + 1:
    the frame grid of the filters) or ``x[f*hop + k] * window[k]`` (F = max(T - W, 0) // hop + 1); x is zero outside [0, T)
    and ``n_frames`` overrides F.  ``a`` are the coefficients of A(z) = 1 + sum_i a_i z^-i that ``ltv_allpole_ss``,
    ``lti_frames_ola`` and ``ltv_inverse`` take, ``rc`` the reflection coefficients with ``rc2lpc(rc) == a``,
    ``gain = sqrt(prediction error / sum(window**2))``.  The zero lag is regularised as ``r0 * (1 + eps_rel) + eps_abs``.
    Lags and recursion run in fp64 on the device; differentiable w.r.t. x through any subset of the outputs (the window is
    a constant).  1 <= order <= 64, order < W <= 4096, hop >= 1."""
    if x.dim() != 2 or window.dim() != 1:
        raise _lib.GolfError(f"lpc_analysis: x must be (B, T) and window (W,) (got {tuple(x.shape)}, {tuple(window.shape)})")
    hop, M, W = int(hop), int(order), window.numel()
    if hop < 1:
        raise _lib.GolfError(f"lpc_analysis: hop={hop} must be >= 1")
    F = lpc_analysis_frames(x.shape[1], W, hop, centred) if n_frames is None else int(n_frames)
    if F < 1:
        raise _lib.GolfError(f"lpc_analysis: n_frames={F} must be >= 1")
    if x.shape[0] * F >= 2 ** 31:   # the library refuses it too; here before the outputs are allocated
        raise _lib.GolfError(f"lpc_analysis: B*F = {x.shape[0] * F} frames, must be < 2^31")
    if x.shape[0] == 0:
        # an empty batch: empty results of the right widths that stay in the graph, like the filters'
        _lib.require_device(x.float(), window)
        z = x.float().sum(1)
        out = (z[:, None].expand(0, F), z[:, None, None].expand(0, F, M), z[:, None, None].expand(0, F, M))
        return out if return_rc else out[:2]
    return _LPCAnalysis.apply(x, window, hop, M, -(W // 2) if centred else 0, F, float(eps_rel), float(eps_abs),
                              bool(return_rc))


@_amp_no_grad   # an analysis without a backward: inference only, like ltv_residual
def _source_filter_lpc(x, window, hop, M, Q, iterations, preemphasis, origin, F, eps_rel, eps_abs, want_rc, want_source):
    _lib.require_device(x, window)
    lib = _lib.load()
    x, window = _rows(x), window.contiguous()
    B, T = x.shape
    gain = torch.empty(B, F, dtype=torch.float32, device=x.device)
    a = torch.empty(B, F, M, dtype=torch.float32, device=x.device)
    rc = torch.empty(B, F, M, dtype=torch.float32, device=x.device) if want_rc else None   # not asked for: not written
    source = torch.empty(B, F, Q, dtype=torch.float32, device=x.device) if want_source else None
    rcode = lib.golf_lpc_source_filter_f32(x.data_ptr(), x.stride(0), window.data_ptr(), gain.data_ptr(), a.data_ptr(),
                                           _lib.ptr(rc), _lib.ptr(source), B, T, F, M, Q, iterations, preemphasis is None,
                                           0.0 if preemphasis is None else preemphasis, hop, window.numel(), origin, eps_rel,
                                           eps_abs, _lib.stream_ptr())
    _lib.check(rcode, "golf_lpc_source_filter_f32")
    return (gain, a) + ((rc,) if want_rc else ()) + ((source,) if want_source else ())


def source_filter_lpc(x: torch.Tensor, window: torch.Tensor, hop: int, order: int, source_order: int = 4, iterations: int = 2,
                      preemphasis: float = None, centred: bool = True, n_frames: int = None, eps_rel: float = 1e-9,
                      eps_abs: float = 1e-12, return_rc: bool = False, return_source: bool = False):
    """Source-compensated LPC analysis (golf_lpc_source_filter_f32, the definition is in include/golf_amd.h): x (B, T),
    window (W,) -> ``(gain (B, F), a (B, F, order))``, then ``rc (B, F, order)`` with ``return_rc`` and ``source (B, F,
    source_order)`` with ``return_source``, on the frames of ``lpc_analysis``.  Iterative adaptive inverse filtering on the
    frame's lags: a first source polynomial of order 1 (``-r[1] / r[0]``, or ``-preemphasis`` when that is given), then
    ``iterations`` rounds of tract (``order``) against source (``source_order``), then the tract once more: ``a`` is the vocal
    tract without the glottal source's spectral tilt, which the GOLF decoders keep in the wavetable, and ``gain`` the level of
    the audio through ``a``'s inverse alone, so that ``ltv_residual(x, gain, a, hop)`` has unit local power.
    ``preemphasis=0, iterations=0`` is ``lpc_analysis``.  Lags and every stage run in fp64 on the device.  No gradient: the
    outputs never require grad; strided rows of x are read in place.  1 <= order <= 64, 1 <= source_order <= 16,
    0 <= iterations <= 8, order + source_order < W <= 4096, hop >= 1, |preemphasis| < 1."""
    who = "source_filter_lpc"
    if x.dim() != 2 or window.dim() != 1:
        raise _lib.GolfError(f"{who}: x must be (B, T) and window (W,) (got {tuple(x.shape)}, {tuple(window.shape)})")
    hop, M, Q, W = int(hop), int(order), int(source_order), window.numel()
    if hop < 1:
        raise _lib.GolfError(f"{who}: hop={hop} must be >= 1")
    F = lpc_analysis_frames(x.shape[1], W, hop, centred) if n_frames is None else int(n_frames)
    if F < 1:
        raise _lib.GolfError(f"{who}: n_frames={F} must be >= 1")
    if x.shape[0] * F >= 2 ** 31:   # the library refuses it too; here before the outputs are allocated
        raise _lib.GolfError(f"{who}: B*F = {x.shape[0] * F} frames, must be < 2^31")
    # (an empty batch goes the same way: the library checks its arguments and launches nothing)
    return _source_filter_lpc(x, window, hop, M, Q, int(iterations), None if preemphasis is None else float(preemphasis),
                              -(W // 2) if centred else 0, F, float(eps_rel), float(eps_abs), bool(return_rc),
                              bool(return_source))


# ------------------------------------------------------------------------------------------------
# f0 analysis: audio -> (f0, period, aperiodicity) per frame by YIN (include/golf_amd.h, csrc/f0_yin.hip)
# ------------------------------------------------------------------------------------------------
F0_MAX_FRAME = 16384   # W + tau_max samples of one frame (csrc/f0_yin.hip YIN_MAX_S)


def f0_frames(T: int, S: int, hop: int, centred: bool = True) -> int:
    """Frames of the f0 analysis for frames of ``S = W + tau_max`` samples: ``T // hop + 1`` centred (the filters' frame
    grid), ``max(T - S, 0) // hop + 1`` for frames that start at sample 0."""
    return lpc_analysis_frames(T, S, hop, centred)


def f0_lags(sample_rate: float, f0_min: float = 60.0, f0_max: float = 1000.0, window_length: int = None):
    """``(tau_min, tau_max, W)`` of the f0 analysis: ``floor(sr / f0_max)``, ``ceil(sr / f0_min)`` and the integration window,
    two of the longest periods unless ``window_length`` is given."""
    if not (sample_rate > 0 and 0 < f0_min < f0_max):
        raise _lib.GolfError(f"f0_yin: need sample_rate > 0 and 0 < f0_min < f0_max (got {sample_rate}, {f0_min}, {f0_max})")
    tau_min, tau_max = int(math.floor(sample_rate / f0_max)), int(math.ceil(sample_rate / f0_min))
    return tau_min, tau_max, 2 * tau_max if window_length is None else int(window_length)


def _f0_frame_grid(who, x, sample_rate, hop, f0_min, f0_max, window_length, centred, n_frames):
    """What ``f0_yin`` and ``f0_candidates`` share: ``(tau_min, tau_max, W, S, origin, F)`` of x (B, T), after every refusal
    that the two have in common."""
    if x.dim() != 2:
        raise _lib.GolfError(f"{who}: x must be (B, T) (got {tuple(x.shape)})")
    if hop < 1:
        raise _lib.GolfError(f"{who}: hop={hop} must be >= 1")
    tau_min, tau_max, W = f0_lags(float(sample_rate), float(f0_min), float(f0_max), window_length)
    if tau_min < 1 or tau_max <= tau_min:
        raise _lib.GolfError(f"{who}: lags {tau_min}..{tau_max} (need 1 <= tau_min < tau_max: f0_max <= sample_rate, "
                             "f0_min < f0_max)")
    if W < 1:
        raise _lib.GolfError(f"{who}: window_length={W} must be >= 1")
    S = W + tau_max
    if S > F0_MAX_FRAME:
        raise _lib.GolfError(f"{who}: frame window_length + tau_max = {S} samples exceeds {F0_MAX_FRAME}")
    F = f0_frames(x.shape[1], S, hop, centred) if n_frames is None else int(n_frames)
    if F < 1:
        raise _lib.GolfError(f"{who}: n_frames={F} must be >= 1")
    if x.shape[0] * F >= 2 ** 31:   # the library refuses it too; here before the outputs are allocated
        raise _lib.GolfError(f"{who}: B*F = {x.shape[0] * F} frames, must be < 2^31")
    return tau_min, tau_max, W, S, -(S // 2) if centred else 0, F


@_amp_no_grad   # a search over lags: no gradient reaches the waveform
def _f0_yin(x, sample_rate, hop, W, tau_min, tau_max, origin, F, threshold, rms_floor, want_all):
    _lib.require_device(x)
    lib = _lib.load()
    x = _rows(x)
    B, T = x.shape
    f0 = torch.empty(B, F, dtype=torch.float32, device=x.device)
    period = torch.empty_like(f0) if want_all else None   # not asked for: not written
    ap = torch.empty_like(f0) if want_all else None
    rcode = lib.golf_f0_yin_f32(x.data_ptr(), x.stride(0), f0.data_ptr(), _lib.ptr(period), _lib.ptr(ap), B, T, F, hop, W,
                                tau_min, tau_max, origin, sample_rate, threshold, rms_floor, _lib.stream_ptr())
    _lib.check(rcode, "golf_f0_yin_f32")
    return (f0, period, ap) if want_all else f0


def f0_yin(x: torch.Tensor, sample_rate: float, hop: int, f0_min: float = 60.0, f0_max: float = 1000.0,
           window_length: int = None, threshold: float = 0.15, rms_floor: float = 0.0, centred: bool = True,
           n_frames: int = None, return_all: bool = False):
    """f0 by YIN (de Cheveigne & Kawahara 2002, steps 1-5; the definition is in include/golf_amd.h): x (B, T) -> ``f0 (B, F)``
    in Hz with 0 for unvoiced frames, or with ``return_all`` ``(f0, period, ap)``: the refined period in samples (finite in
    every frame) and the aperiodicity d'(period), small for a periodic frame and about 1 for noise.  Lags run from
    ``floor(sample_rate / f0_max)`` to ``tau_max = ceil(sample_rate / f0_min)`` and the difference function integrates over
    ``window_length`` samples (default ``2 * tau_max``), so frame f reads ``S = window_length + tau_max`` samples from
    ``f * hop - S // 2`` (``centred``, F = T // hop + 1: the frame grid of the filters and of ``lpc_analysis``) or from
    ``f * hop`` (F = max(T - S, 0) // hop + 1); x is zero outside [0, T) and ``n_frames`` overrides F.  A frame is voiced
    if a lag falls below ``threshold`` and its RMS over the window exceeds ``rms_floor``.  The outputs never require grad;
    a waveform that does is accepted.  S <= 16384."""
    hop = int(hop)
    tau_min, tau_max, W, S, origin, F = _f0_frame_grid("f0_yin", x, sample_rate, hop, f0_min, f0_max, window_length, centred,
                                                       n_frames)
    if x.shape[0] == 0:
        _lib.require_device(x.float())
        z = torch.empty(0, F, dtype=torch.float32, device=x.device)
        return (z, z.clone(), z.clone()) if return_all else z
    return _f0_yin(x, float(sample_rate), hop, W, tau_min, tau_max, origin, F, float(threshold), float(rms_floor),
                   bool(return_all))


# ------------------------------------------------------------------------------------------------
# harmonic-plus-noise analysis: (audio, f0) -> harmonic amplitudes, phases and noise-filter log magnitudes per frame
# (include/golf_amd.h, csrc/harm_analysis.hip)
# ------------------------------------------------------------------------------------------------
HNA_MAX_WINDOW = 2048      # csrc/harm_analysis.hip HNA_MAX_L
HNA_MAX_HARMONICS = 256    # HNA_MAX_K
HNA_MAX_NMAG = 513         # HNA_MAX_NMAG


@_amp_no_grad   # an analysis without a backward: inference only, like f0_yin
def _harmonic_analysis(x, f0, pos, n_frames, sample_rate, params, eps, want_phases):
    """``pos``: None for the one-shot entry, ``(x_t0, f_first, f0_first, last)`` for the stream entry; ``params``: what
    ``_hna_params`` returns."""
    hop, K, n_mag, periods, min_window, max_window, unvoiced_window, smooth = params
    _lib.require_device(x, f0)
    lib = _lib.load()
    x, f0 = _rows(x), _rows(f0)
    B = x.shape[0]
    amp = torch.empty(B, n_frames, K, dtype=torch.float32, device=x.device)
    phases = torch.empty_like(amp) if want_phases else None   # not asked for: not written
    log_mag = torch.empty(B, n_frames, n_mag, dtype=torch.float32, device=x.device) if n_mag else None
    if pos is None:
        rcode = lib.golf_harmonic_analysis_f32(x.data_ptr(), x.stride(0), f0.data_ptr(), f0.stride(0), amp.data_ptr(),
                                               _lib.ptr(phases), _lib.ptr(log_mag), B, x.shape[1], n_frames, K, n_mag, hop,
                                               periods, min_window, max_window, unvoiced_window, smooth, sample_rate, eps,
                                               _lib.stream_ptr())
        _lib.check(rcode, "golf_harmonic_analysis_f32")
    else:
        x_t0, f_first, f0_first, last = pos
        rcode = lib.golf_harmonic_analysis_stream_f32(x.data_ptr(), x.stride(0), x_t0, x.shape[1], f0.data_ptr(),
                                                      f0.stride(0), f0_first, f0.shape[1], amp.data_ptr(), _lib.ptr(phases),
                                                      _lib.ptr(log_mag), B, f_first, n_frames, int(last), K, n_mag, hop,
                                                      periods, min_window, max_window, unvoiced_window, smooth, sample_rate,
                                                      eps, _lib.stream_ptr())
        _lib.check(rcode, "golf_harmonic_analysis_stream_f32")
    return tuple(t for t in (amp, phases, log_mag) if t is not None)


def _hna_result(x, f0, pos, n_frames, sample_rate, params, eps, return_phases):
    """What either entry returns once its checks have passed: empty results without a launch for an empty batch or no frame."""
    if x.shape[0] == 0 or n_frames == 0:
        K, n_mag = params[1:3]
        _lib.require_device(x.float(), f0.float())
        out = [torch.empty(x.shape[0], n_frames, K, dtype=torch.float32, device=x.device)]
        if return_phases:
            out.append(out[0].clone())
        if n_mag:
            out.append(torch.empty(x.shape[0], n_frames, n_mag, dtype=torch.float32, device=x.device))
    else:
        out = _harmonic_analysis(x, f0, pos, n_frames, float(sample_rate), params, float(eps), bool(return_phases))
    return out[0] if len(out) == 1 else tuple(out)


def _check_frame_position(who, x, f0, x_t0, f_first, f0_first, n_frames, last, hop, back, ahead, f_back, f_ahead) -> None:
    """The position of a frame analysis' stream entry: frames ``f_first .. f_first + n_frames - 1``, of which frame f may read
    the samples ``[f hop - back, f hop + ahead)`` and the f0 frames ``f - f_back .. f + f_ahead``, from x (B, n_x), the samples
    from ``x_t0`` on, and f0 (B, n_f0), the frames from ``f0_first`` on.  What lies beyond the buffers is read only by a
    ``last`` call."""
    (B, n_x), n_f0 = x.shape, f0.shape[1]
    _check_frames(who, "n_frames", n_frames, 0, B)
    _check_far(who, hop, "f_first", f_first, "n_frames", n_frames, "x_t0", x_t0, "f0_first", f0_first)
    if not n_frames:
        return
    lo, f_lo, f_end, x_end, f0_end = max(f_first * hop - back, 0), max(f_first - f_back, 0), f_first + n_frames, x_t0 + n_x, \
        f0_first + n_f0
    if x_t0 > lo:
        raise _lib.GolfError(f"{who}: x_t0={x_t0} lies above sample {lo}, where the window of frame f_first={f_first} may "
                             "start")
    if f0_first > f_lo:
        raise _lib.GolfError(f"{who}: f0_first={f0_first} lies above frame {f_lo}, the first that frame f_first={f_first} "
                             "reads")
    if f_end > f0_end:
        raise _lib.GolfError(f"{who}: f0 ends at frame {f0_end} (n_f0={n_f0}), before the last computed frame {f_end - 1}")
    if not last and (f_end - 1) * hop + ahead > x_end:
        raise _lib.GolfError(f"{who}: x ends at sample {x_end} (n_x={n_x}), before the window of frame {f_end - 1} may end "
                             f"({(f_end - 1) * hop + ahead}), and last is not set")
    if not last and f_end + f_ahead > f0_end:   # (f_ahead = 0: the check before this one has made it)
        raise _lib.GolfError(f"{who}: f0 ends at frame {f0_end} (n_f0={n_f0}), without the neighbour after frame "
                             f"{f_end - 1}, and last is not set")


def harmonic_analysis(x: torch.Tensor, f0: torch.Tensor, sample_rate: float, hop: int, num_harmonics: int,
                      n_mag: int = None, periods: int = 4, min_window: int = None, max_window: int = 2048,
                      unvoiced_window: int = None, smooth: int = 0, eps: float = 1e-12, return_phases: bool = False):
    """Harmonic-plus-noise analysis (the definition is in include/golf_amd.h): x (B, T) and its f0 track (B, F) in Hz, 0 where
    unvoiced, frame f centred on sample ``f * hop`` -> ``amplitudes (B, F, num_harmonics)``, what ``harmonic_osc`` takes as
    ``amp`` at hop ``hop`` with the phase ``f0 / sample_rate``; with ``n_mag`` also ``log_mag (B, F, n_mag)``, what
    ``zero_phase_fir_filter`` takes for N(0, 1) noise; with ``return_phases`` the sine phases in cycles at the frames'
    centres, second in the tuple: ``amplitudes``, ``(amplitudes, log_mag)``, ``(amplitudes, phases)`` or ``(amplitudes,
    phases, log_mag)``.  A voiced frame's window is a whole number of periods, at least ``periods`` and at least about
    ``min_window`` (default ``2 * hop``) samples, at most ``max_window`` <= 2048; an unvoiced frame's is ``unvoiced_window``
    (default ``4 * hop``) <= 2048.  ``smooth`` averages the noise power over ``2 * smooth + 1`` bins.  Harmonics at or above
    Nyquist are 0; x is 0 outside [0, T).  The outputs never require grad; strided rows are read in place."""
    who = "harmonic_analysis"
    params = _hna_params(who, x, f0, sample_rate, hop, num_harmonics, n_mag, periods, min_window, max_window, unvoiced_window,
                         smooth, eps)
    B, F = f0.shape
    _check_frames(who, "F", F, 1, B)
    return _hna_result(x, f0, None, F, sample_rate, params, eps, return_phases)


def _hna_params(who, x, f0, sample_rate, hop, num_harmonics, n_mag, periods, min_window, max_window, unvoiced_window, smooth,
                eps):
    """The argument checks the two entries share; the integers with their defaults filled in, in the order in which
    ``_harmonic_analysis`` takes them."""
    hop = _analysis_head(who, x, f0, "f0", hop, sample_rate)
    K, periods, smooth = int(num_harmonics), int(periods), int(smooth)
    n_mag = 0 if n_mag is None else int(n_mag)
    min_window = 2 * hop if min_window is None else int(min_window)
    unvoiced_window = 4 * hop if unvoiced_window is None else int(unvoiced_window)
    max_window = int(max_window)
    if not 1 <= K <= HNA_MAX_HARMONICS:
        raise _lib.GolfError(f"{who}: num_harmonics={K} must be 1..{HNA_MAX_HARMONICS}")
    if n_mag and not 2 <= n_mag <= HNA_MAX_NMAG:
        raise _lib.GolfError(f"{who}: n_mag={n_mag} must be 2..{HNA_MAX_NMAG} (or None)")
    if periods < 2:
        raise _lib.GolfError(f"{who}: periods={periods} must be >= 2")
    if not 2 <= max_window <= HNA_MAX_WINDOW or not 2 <= unvoiced_window <= HNA_MAX_WINDOW:
        raise _lib.GolfError(f"{who}: max_window={max_window} and unvoiced_window={unvoiced_window} must be "
                             f"2..{HNA_MAX_WINDOW}")
    if not 1 <= min_window <= max_window:
        raise _lib.GolfError(f"{who}: min_window={min_window} must be 1..max_window={max_window}")
    if smooth < 0 or (n_mag and smooth >= n_mag):
        raise _lib.GolfError(f"{who}: smooth={smooth} must be 0..n_mag-1 (n_mag={n_mag})")
    if not eps >= 0:
        raise _lib.GolfError(f"{who}: eps={eps} must be >= 0")
    return hop, K, n_mag, periods, min_window, max_window, unvoiced_window, smooth


def harmonic_analysis_stream(x: torch.Tensor, f0: torch.Tensor, x_t0: int, f_first: int, f0_first: int, n_frames: int,
                             last: bool, sample_rate: float, hop: int, num_harmonics: int, n_mag: int = None,
                             periods: int = 4, min_window: int = None, max_window: int = 2048, unvoiced_window: int = None,
                             smooth: int = 0, eps: float = 1e-12, return_phases: bool = False):
    """``harmonic_analysis`` at a position of a longer utterance (golf_harmonic_analysis_stream_f32, include/golf_amd.h):
    frames ``f_first .. f_first + n_frames - 1`` from x (B, n_x), the utterance's samples ``[x_t0, x_t0 + n_x)``, and f0
    (B, n_f0), its frames ``[f0_first, f0_first + n_f0)``; ``last``: the utterance ends with these buffers.  The results are
    those of ``harmonic_analysis`` with ``n_frames`` in place of F, and each frame has the bits the one-shot call gives it.
    With ``Lmax = max(max_window, unvoiced_window)`` the buffers must hold what the frames can read: ``0 <= x_t0 <=
    max(0, f_first * hop - Lmax // 2)``, ``0 <= f0_first <= max(f_first - 1, 0)``, ``f_first + n_frames <= f0_first + n_f0``
    and, unless ``last``, ``(f_first + n_frames - 1) * hop + Lmax - Lmax // 2 <= x_t0 + n_x`` and ``f_first + n_frames + 1 <=
    f0_first + n_f0``; anything else raises ``GolfError`` before a launch.  ``n_frames = 0`` or an empty batch returns empty
    results without a launch."""
    who = "harmonic_analysis_stream"
    hop, _, _, _, _, max_window, unvoiced_window, _ = params = _hna_params(
        who, x, f0, sample_rate, hop, num_harmonics, n_mag, periods, min_window, max_window, unvoiced_window, smooth, eps)
    x_t0, f_first, f0_first, n_frames, last = int(x_t0), int(f_first), int(f0_first), int(n_frames), bool(last)
    Lmax = max(max_window, unvoiced_window)
    _check_frame_position(who, x, f0, x_t0, f_first, f0_first, n_frames, last, hop, Lmax // 2, Lmax - Lmax // 2, 1, 1)
    return _hna_result(x, f0, (x_t0, f_first, f0_first, last), n_frames, sample_rate, params, eps, return_phases)


ENV_MIN_NFFT, ENV_MAX_NFFT = 64, 2048   # csrc/spec_envelope.hip ENV_MIN_N, ENV_MAX_N
ENV_VOICED_OFFSET = 0.5 * math.log(2.0)


@_amp_no_grad   # an analysis without a backward: inference only, like harmonic_analysis
def _spectral_envelope(x, f0, pos, n_frames, sample_rate, params, unvoiced_f0, q1, eps, voiced_offset, want_env):
    """``pos``: None for the one-shot entry, ``(x_t0, f_first, f0_first, last)`` for the stream entry; ``params``: what
    ``_env_params`` returns."""
    hop, n_fft, n_ceps, _, f0_floor, f0_ceil = params
    _lib.require_device(x, f0)
    lib = _lib.load()
    x, f0 = _rows(x), _rows(f0)
    B = x.shape[0]
    log_env = torch.empty(B, n_frames, n_fft // 2 + 1, dtype=torch.float32, device=x.device) if want_env else None
    ceps = torch.empty(B, n_frames, n_ceps, dtype=torch.float32, device=x.device) if n_ceps else None   # not asked for: not written
    if pos is None:
        rcode = lib.golf_spectral_envelope_f32(x.data_ptr(), x.stride(0), f0.data_ptr(), f0.stride(0), _lib.ptr(log_env),
                                               _lib.ptr(ceps), B, x.shape[1], n_frames, n_fft, n_ceps, hop, sample_rate,
                                               f0_floor, f0_ceil, unvoiced_f0, q1, eps, voiced_offset, _lib.stream_ptr())
        _lib.check(rcode, "golf_spectral_envelope_f32")
    else:
        x_t0, f_first, f0_first, last = pos
        rcode = lib.golf_spectral_envelope_stream_f32(x.data_ptr(), x.stride(0), x_t0, x.shape[1], f0.data_ptr(),
                                                      f0.stride(0), f0_first, f0.shape[1], _lib.ptr(log_env), _lib.ptr(ceps),
                                                      B, f_first, n_frames, int(last), n_fft, n_ceps, hop, sample_rate,
                                                      f0_floor, f0_ceil, unvoiced_f0, q1, eps, voiced_offset,
                                                      _lib.stream_ptr())
        _lib.check(rcode, "golf_spectral_envelope_stream_f32")
    return tuple(t for t in (log_env, ceps) if t is not None)


def _env_result(x, f0, pos, n_frames, sample_rate, params, unvoiced_f0, q1, eps, voiced_offset, return_log_env):
    """What either entry returns once its checks have passed: empty results without a launch for an empty batch or no frame."""
    if x.shape[0] == 0 or n_frames == 0:
        n_ceps, nb = params[2:4]
        _lib.require_device(x.float(), f0.float())
        out = [torch.empty(x.shape[0], n_frames, w, dtype=torch.float32, device=x.device)
               for w, want in ((nb, return_log_env), (n_ceps, n_ceps)) if want]
    else:
        out = _spectral_envelope(x, f0, pos, n_frames, float(sample_rate), params, float(unvoiced_f0), float(q1), float(eps),
                                 float(voiced_offset), bool(return_log_env))
    return out[0] if len(out) == 1 else tuple(out)


def spectral_envelope_defaults(sample_rate: float, n_fft: int = 1024):
    """``(f0_floor, f0_ceil)`` that ``spectral_envelope`` takes when they are None: the lowest f0 whose three-period window
    fits the transform, ``3 sr / (n_fft - 3)`` (70.5 Hz at 24 kHz and 1024), and ``sr / 12``."""
    return 3.0 * sample_rate / (n_fft - 3), sample_rate / 12.0


def _env_params(who, x, f0, sample_rate, hop, n_fft, n_ceps, f0_floor, f0_ceil, unvoiced_f0, q1, eps, voiced_offset,
                return_log_env):
    """The argument checks the two entries share; the numbers with their defaults filled in."""
    hop, n_fft = _analysis_head(who, x, f0, "f0", hop, sample_rate), int(n_fft)
    n_ceps = 0 if n_ceps is None else int(n_ceps)
    if not ENV_MIN_NFFT <= n_fft <= ENV_MAX_NFFT or n_fft & (n_fft - 1):
        raise _lib.GolfError(f"{who}: n_fft={n_fft} must be a power of two in [{ENV_MIN_NFFT}, {ENV_MAX_NFFT}]")
    nb = n_fft // 2 + 1
    if not 0 <= n_ceps <= nb:
        raise _lib.GolfError(f"{who}: n_ceps={n_ceps} must be 1..{nb} (or None)")
    if not n_ceps and not return_log_env:
        raise _lib.GolfError(f"{who}: nothing to return: n_ceps is None and return_log_env is False")
    lo, hi = spectral_envelope_defaults(float(sample_rate), n_fft)
    f0_floor, f0_ceil = lo if f0_floor is None else float(f0_floor), hi if f0_ceil is None else float(f0_ceil)
    if not f0_floor > 0 or not f0_floor <= f0_ceil:
        raise _lib.GolfError(f"{who}: f0_floor={f0_floor} must be positive and <= f0_ceil={f0_ceil}")
    if not f0_ceil <= sample_rate / 4:
        raise _lib.GolfError(f"{who}: f0_ceil={f0_ceil} must be <= sample_rate/4 = {sample_rate / 4}")
    if not f0_floor <= unvoiced_f0 <= f0_ceil:
        raise _lib.GolfError(f"{who}: unvoiced_f0={unvoiced_f0} must lie in [f0_floor, f0_ceil] = [{f0_floor}, {f0_ceil}]")
    if math.floor(1.5 * sample_rate / f0_floor + 0.5) > n_fft // 2 - 1:
        raise _lib.GolfError(f"{who}: f0_floor={f0_floor}: the longest window, 2*"
                             f"{math.floor(1.5 * sample_rate / f0_floor + 0.5)} + 1 samples, must fit n_fft={n_fft}")
    if not eps > 0:
        raise _lib.GolfError(f"{who}: eps={eps} must be positive")
    if q1 != q1 or voiced_offset != voiced_offset:
        raise _lib.GolfError(f"{who}: q1={q1} and voiced_offset={voiced_offset} must be numbers")
    return hop, n_fft, n_ceps, nb, f0_floor, f0_ceil


def spectral_envelope(x: torch.Tensor, f0: torch.Tensor, sample_rate: float, hop: int, n_fft: int = 1024,
                      n_ceps: int = None, f0_floor: float = None, f0_ceil: float = None, unvoiced_f0: float = 500.0,
                      q1: float = -0.15, eps: float = 1e-12, voiced_offset: float = ENV_VOICED_OFFSET,
                      return_log_env: bool = True):
    """Pitch-adaptive spectral-envelope analysis (the definition is in include/golf_amd.h): x (B, T) and its f0 track (B, F)
    in Hz, 0 where unvoiced, frame f centred on sample ``f * hop`` -> ``log_env (B, F, n_fft/2 + 1)``, the natural log of the
    magnitude envelope on bins 0 .. n_fft/2 (``exp`` of it is what ``stft_filter_frames`` takes as response rows); with
    ``n_ceps`` also ``ceps (B, F, n_ceps)`` in ``LTVCepFilter``'s convention (``n_ceps = filter_order + 1``); with
    ``return_log_env=False`` ``ceps`` alone: ``log_env``, ``ceps`` or ``(log_env, ceps)``.  A frame's window is three periods
    of its f0 clamped to [``f0_floor``, ``f0_ceil``] (defaults ``spectral_envelope_defaults``), of ``unvoiced_f0`` where
    unvoiced; ``voiced_offset`` (default ``0.5 ln 2``) is added to the log magnitude of voiced frames, which makes them
    return log|H| of the filter an ``AdditivePulseTrain`` went through.  x is 0 outside [0, T).  The outputs never require
    grad; strided rows are read in place."""
    who = "spectral_envelope"
    params = _env_params(who, x, f0, sample_rate, hop, n_fft, n_ceps, f0_floor, f0_ceil, unvoiced_f0, q1, eps, voiced_offset,
                         return_log_env)
    B, F = f0.shape
    _check_frames(who, "F", F, 1, B)
    return _env_result(x, f0, None, F, sample_rate, params, unvoiced_f0, q1, eps, voiced_offset, return_log_env)


def spectral_envelope_hwmax(sample_rate: float, n_fft: int = 1024, f0_floor: float = None) -> int:
    """The longest half window a frame of ``spectral_envelope`` can take, ``floor(1.5 sr / f0_floor + 0.5)`` samples."""
    lo = spectral_envelope_defaults(float(sample_rate), int(n_fft))[0] if f0_floor is None else float(f0_floor)
    return math.floor(1.5 * float(sample_rate) / lo + 0.5)


def spectral_envelope_stream(x: torch.Tensor, f0: torch.Tensor, x_t0: int, f_first: int, f0_first: int, n_frames: int,
                             last: bool, sample_rate: float, hop: int, n_fft: int = 1024, n_ceps: int = None,
                             f0_floor: float = None, f0_ceil: float = None, unvoiced_f0: float = 500.0, q1: float = -0.15,
                             eps: float = 1e-12, voiced_offset: float = ENV_VOICED_OFFSET, return_log_env: bool = True):
    """``spectral_envelope`` at a position of a longer utterance (golf_spectral_envelope_stream_f32, include/golf_amd.h):
    frames ``f_first .. f_first + n_frames - 1`` from x (B, n_x), the utterance's samples ``[x_t0, x_t0 + n_x)``, and f0
    (B, n_f0), its frames ``[f0_first, f0_first + n_f0)``; ``last``: the utterance ends with the x buffer.  The results are
    those of ``spectral_envelope`` with ``n_frames`` in place of F, and each frame has the bits the one-shot call gives it.
    With ``hwmax = spectral_envelope_hwmax(sample_rate, n_fft, f0_floor)`` the buffers must hold what the frames can read:
    ``0 <= x_t0 <= max(0, f_first * hop - hwmax)``, ``f0_first <= f_first``, ``f_first + n_frames <= f0_first + n_f0`` and,
    unless ``last``, ``(f_first + n_frames - 1) * hop + hwmax + 1 <= x_t0 + n_x``; anything else raises ``GolfError`` before a
    launch.  ``n_frames = 0`` or an empty batch returns empty results without a launch."""
    who = "spectral_envelope_stream"
    hop, _, _, _, f0_floor, _ = params = _env_params(who, x, f0, sample_rate, hop, n_fft, n_ceps, f0_floor, f0_ceil,
                                                         unvoiced_f0, q1, eps, voiced_offset, return_log_env)
    x_t0, f_first, f0_first, n_frames, last = int(x_t0), int(f_first), int(f0_first), int(n_frames), bool(last)
    hwmax = math.floor(1.5 * float(sample_rate) / f0_floor + 0.5)   # spectral_envelope_hwmax at the f0_floor in force
    _check_frame_position(who, x, f0, x_t0, f_first, f0_first, n_frames, last, hop, hwmax, hwmax + 1, 0, 0)
    return _env_result(x, f0, (x_t0, f_first, f0_first, last), n_frames, sample_rate, params, unvoiced_f0, q1, eps,
                       voiced_offset, return_log_env)


# ------------------------------------------------------------------------------------------------
# glottal-source analysis: a residual's harmonics against the glottal-flow wavetable (csrc/glottal_match.hip)
# ------------------------------------------------------------------------------------------------
GLOTTAL_MAX_HARMONICS, GLOTTAL_MAX_ROWS = 256, 1024   # csrc/glottal_match.hip GM_MAX_H, GM_MAX_K
GLOTTAL_MIN_NPHI, GLOTTAL_MAX_NPHI = 8, 4096          # GM_MIN_NPHI, GM_MAX_NPHI


@dataclasses.dataclass(frozen=True)
class GlottalPlan:
    """What ``glottal_match`` needs of a table (K, L), built once per table by ``glottal_plan``: ``spectrum`` (K, H, 2),
    ``norms`` (K, H) and ``cross`` (K - 1, H), fp32 and contiguous (include/golf_amd.h golf_glottal_match_f32)."""
    spectrum: torch.Tensor
    norms: torch.Tensor
    cross: torch.Tensor


def glottal_plan(table: torch.Tensor, num_harmonics: int) -> GlottalPlan:
    """The plan of a wavetable (K, L) for ``num_harmonics`` harmonics, in stock torch on the table's device (a CPU table
    gives a CPU plan): S[k,h] = 2 rfft(table[k])[h] / L for h = 1..H, zero for h > L/2, transformed in float64 and stored in
    fp32; the prefix sums N[k,h] = sum_{i<=h} |S[k,i]|^2 and X[k,h] = sum_{i<=h} Re(S[k,i] conj(S[k+1,i])) of the stored S,
    summed in float64 and stored in fp32.  Never requires grad."""
    who = "glottal_plan"
    H = int(num_harmonics)
    if table.dim() != 2:
        raise _lib.GolfError(f"{who}: the table must be (K, L) (got {tuple(table.shape)})")
    K, L = table.shape
    if not 2 <= K <= GLOTTAL_MAX_ROWS:
        raise _lib.GolfError(f"{who}: the table has {K} rows, must be 2..{GLOTTAL_MAX_ROWS}")
    if L < 2:
        raise _lib.GolfError(f"{who}: the table has {L} points per row, must be >= 2")
    if not 1 <= H <= GLOTTAL_MAX_HARMONICS:
        raise _lib.GolfError(f"{who}: num_harmonics={H} must be 1..{GLOTTAL_MAX_HARMONICS}")
    with torch.no_grad():
        spec = torch.fft.rfft(table.detach().double(), dim=1)[:, 1:H + 1] * (2.0 / L)   # bins 1 .. min(H, L/2)
        S = torch.zeros(K, H, 2, dtype=torch.float32, device=table.device)
        S[:, :spec.shape[1]] = torch.view_as_real(spec).float()
        Sd = S.double()
        N = (Sd * Sd).sum(-1).cumsum(1).float()
        X = (Sd[:-1] * Sd[1:]).sum(-1).cumsum(1).float()
    return GlottalPlan(S.contiguous(), N.contiguous(), X.contiguous())


@_amp_no_grad   # a search: no gradient reaches the harmonics
def _glottal_match(amplitudes, phases, f0, S, N, X, sample_rate, n_phi):
    _lib.require_device(amplitudes, phases, f0, S, N, X)
    lib = _lib.load()
    amplitudes, phases, f0 = amplitudes.contiguous(), phases.contiguous(), _rows(f0)
    B, F, H = amplitudes.shape
    w, theta, rho = (torch.empty(B, F, dtype=torch.float32, device=f0.device) for _ in range(3))
    rcode = lib.golf_glottal_match_f32(amplitudes.data_ptr(), phases.data_ptr(), f0.data_ptr(), f0.stride(0), S.data_ptr(),
                                       N.data_ptr(), X.data_ptr(), w.data_ptr(), theta.data_ptr(), rho.data_ptr(), B, F, H,
                                       S.shape[0], n_phi, sample_rate, _lib.stream_ptr())
    _lib.check(rcode, "golf_glottal_match_f32")
    return w, theta, rho


def glottal_match(amplitudes: torch.Tensor, phases: torch.Tensor, f0: torch.Tensor, plan: GlottalPlan, sample_rate: float,
                  n_phi: int = 256):
    """Match of a residual's harmonics against a glottal-flow wavetable (the definition is in include/golf_amd.h):
    ``amplitudes``, ``phases`` (B, F, H) as ``harmonic_analysis(e, f0, ..., return_phases=True)`` gives them for the residual
    ``e``, its f0 track (B, F) in Hz, 0 where unvoiced, and the table's ``glottal_plan`` for the same H -> ``(w, theta,
    rho)``, (B, F) each: ``w`` in [0, 1] is the position on the table's rows, what ``glottal_osc`` takes as ``wsel`` (NaN in
    an unvoiced frame, a frame without a harmonic below Nyquist and an all-zero frame), ``theta`` in [0, 1) the table phase
    at the frame's centre and ``rho`` in [-1, 1] the normalised correlation of the frame with the chosen pulse (both 0 where
    ``w`` is NaN).  ``n_phi`` phase shifts are searched, a power of two in [8, 4096].  The outputs never require grad;
    strided ``f0`` rows are read in place."""
    who = "glottal_match"
    if not isinstance(plan, GlottalPlan):
        raise _lib.GolfError(f"{who}: plan must be a GlottalPlan (glottal_plan(table, num_harmonics))")
    if amplitudes.dim() != 3 or phases.shape != amplitudes.shape:
        raise _lib.GolfError(f"{who}: amplitudes and phases must be (B, F, H) alike (got {tuple(amplitudes.shape)}, "
                             f"{tuple(phases.shape)})")
    B, F, H = amplitudes.shape
    if f0.dim() != 2 or tuple(f0.shape) != (B, F):
        raise _lib.GolfError(f"{who}: f0 must be (B, F) = {(B, F)} (got {tuple(f0.shape)})")
    S, N, X = plan.spectrum, plan.norms, plan.cross
    K = S.shape[0]
    if S.dim() != 3 or S.shape[2] != 2 or tuple(N.shape) != (K, S.shape[1]) or tuple(X.shape) != (K - 1, S.shape[1]):
        raise _lib.GolfError(f"{who}: the plan's shapes do not go together (spectrum {tuple(S.shape)}, norms "
                             f"{tuple(N.shape)}, cross {tuple(X.shape)})")
    if not all(t.is_contiguous() for t in (S, N, X)):
        raise _lib.GolfError(f"{who}: the plan's tensors must be contiguous")
    if S.shape[1] != H:
        raise _lib.GolfError(f"{who}: the plan was built for {S.shape[1]} harmonics, the analysis has {H}")
    n_phi = int(n_phi)
    if not 1 <= H <= GLOTTAL_MAX_HARMONICS:
        raise _lib.GolfError(f"{who}: H={H} harmonics, must be 1..{GLOTTAL_MAX_HARMONICS}")
    if not 2 <= K <= GLOTTAL_MAX_ROWS:
        raise _lib.GolfError(f"{who}: the plan has {K} rows, must be 2..{GLOTTAL_MAX_ROWS}")
    if not GLOTTAL_MIN_NPHI <= n_phi <= GLOTTAL_MAX_NPHI or n_phi & (n_phi - 1):
        raise _lib.GolfError(f"{who}: n_phi={n_phi} must be a power of two in [{GLOTTAL_MIN_NPHI}, {GLOTTAL_MAX_NPHI}]")
    if not sample_rate > 0:
        raise _lib.GolfError(f"{who}: sample_rate={sample_rate} must be positive")
    if F < 1:
        raise _lib.GolfError(f"{who}: f0 has {F} frames, must be >= 1")
    if B * F >= 2 ** 31:   # the library refuses it too; here before the outputs are allocated
        raise _lib.GolfError(f"{who}: B*F = {B * F} frames, must be < 2^31")
    if B == 0:
        _lib.require_device(amplitudes.float(), phases.float(), f0.float(), S, N, X)
        return tuple(torch.empty(0, F, dtype=torch.float32, device=f0.device) for _ in range(3))
    return _glottal_match(amplitudes, phases, f0, S, N, X, float(sample_rate), n_phi)


# ------------------------------------------------------------------------------------------------
# f0 tracking: per-frame candidate periods (csrc/f0_yin.hip) and the minimum-cost path through them (csrc/f0_viterbi.hip)
# ------------------------------------------------------------------------------------------------
F0_MAX_CANDIDATES = 7      # csrc/f0_yin.hip YIN_MAX_K, csrc/f0_path.h PATH_MAX_K: 8 states, the 64 lanes are their pairs
F0_VITERBI_COSTS = dict(unvoiced_cost=0.3, lag_cost=0.02, jump_cost=0.35, switch_cost=0.14)


@_amp_no_grad   # a search over lags: no gradient reaches the waveform
def _f0_candidates(x, hop, W, tau_min, tau_max, K, origin, F, rms_floor):
    _lib.require_device(x)
    lib = _lib.load()
    x = _rows(x)
    B, T = x.shape
    period = torch.empty(B, F, K, dtype=torch.float32, device=x.device)
    ap = torch.empty_like(period)
    rcode = lib.golf_f0_candidates_f32(x.data_ptr(), x.stride(0), period.data_ptr(), ap.data_ptr(), B, T, F, hop, W,
                                       tau_min, tau_max, K, origin, rms_floor, _lib.stream_ptr())
    _lib.check(rcode, "golf_f0_candidates_f32")
    return period, ap


def f0_candidates(x: torch.Tensor, sample_rate: float, hop: int, f0_min: float = 60.0, f0_max: float = 1000.0,
                  window_length: int = None, n_candidates: int = 7, rms_floor: float = 0.0, centred: bool = True,
                  n_frames: int = None):
    """Candidate periods per frame for ``f0_viterbi`` (the definition is in include/golf_amd.h): x (B, T) ->
    ``(cand_period, cand_ap)``, each (B, F, n_candidates).  The frames, lags and the normalised difference d' are those of
    ``f0_yin``; the candidates are the ``n_candidates`` (1..7) local minima of d' with the smallest values, listed by
    ascending lag and refined like ``f0_yin``'s period.  A slot that is not used holds period 0 and ap +inf; a frame whose
    RMS over the window is at most ``rms_floor`` has none.  The outputs never require grad."""
    hop, K = int(hop), int(n_candidates)
    tau_min, tau_max, W, S, origin, F = _f0_frame_grid("f0_candidates", x, sample_rate, hop, f0_min, f0_max, window_length,
                                                       centred, n_frames)
    if not 1 <= K <= F0_MAX_CANDIDATES:
        raise _lib.GolfError(f"f0_candidates: n_candidates={K} must be 1..{F0_MAX_CANDIDATES}")
    if x.shape[0] == 0:
        _lib.require_device(x.float())
        z = torch.empty(0, F, K, dtype=torch.float32, device=x.device)
        return z, z.clone()
    return _f0_candidates(x, hop, W, tau_min, tau_max, K, origin, F, float(rms_floor))


def _f0_path_shape(who, cand_period, cand_ap, sample_rate, lag_ref):
    """What ``f0_viterbi`` and ``f0_viterbi_stream`` share: ``(B, F, K)`` of the candidates, after every refusal that the two
    have in common."""
    if cand_period.dim() != 3 or cand_period.shape != cand_ap.shape:
        raise _lib.GolfError(f"{who}: cand_period and cand_ap must both be (B, F, K) (got {tuple(cand_period.shape)} and "
                             f"{tuple(cand_ap.shape)})")
    if not 1 <= cand_period.shape[2] <= F0_MAX_CANDIDATES:
        raise _lib.GolfError(f"{who}: K={cand_period.shape[2]} candidates must be 1..{F0_MAX_CANDIDATES}")
    if not (float(sample_rate) > 0 and float(lag_ref) > 0):
        raise _lib.GolfError(f"{who}: sample_rate={sample_rate} and lag_ref={lag_ref} must be positive")
    return cand_period.shape


@_amp_no_grad   # an argmin over paths: no gradient reaches the candidates
def _f0_viterbi(cand_period, cand_ap, sample_rate, lag_ref, unvoiced_cost, lag_cost, jump_cost, switch_cost, want_state):
    _lib.require_device(cand_period, cand_ap)
    lib = _lib.load()
    cand_period, cand_ap = cand_period.contiguous(), cand_ap.contiguous()
    B, F, K = cand_period.shape
    f0 = torch.empty(B, F, dtype=torch.float32, device=cand_period.device)
    state = torch.empty(B, F, dtype=torch.int32, device=cand_period.device) if want_state else None
    ws_bytes = lib.golf_f0_viterbi_workspace_bytes(B, F, K)   # the backpointers of more frames than LDS holds
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=cand_period.device) if ws_bytes else None
    rcode = lib.golf_f0_viterbi_f32(cand_period.data_ptr(), cand_ap.data_ptr(), f0.data_ptr(), _lib.ptr(state),
                                    _lib.ptr(ws), ws_bytes, B, F, K, sample_rate, lag_ref, unvoiced_cost, lag_cost,
                                    jump_cost, switch_cost, _lib.stream_ptr())
    _lib.check(rcode, "golf_f0_viterbi_f32")
    return (f0, state) if want_state else f0


def f0_viterbi(cand_period: torch.Tensor, cand_ap: torch.Tensor, sample_rate: float, lag_ref: float,
               unvoiced_cost: float = 0.3, lag_cost: float = 0.02, jump_cost: float = 0.35, switch_cost: float = 0.14,
               return_state: bool = False):
    """The minimum-cost path through the candidates of ``f0_candidates`` (B, F, K), K <= 7, over each row (the definition is
    in include/golf_amd.h): ``f0 (B, F)`` in Hz with 0 for the frames the path calls unvoiced, or with ``return_state``
    ``(f0, state)``, state (B, F) int32 with 0 for unvoiced and k + 1 for slot k.  A frame costs ``unvoiced_cost`` unvoiced
    and ``max(ap, 0) + lag_cost * log2(period / lag_ref)`` on a candidate; a step between two candidates costs ``jump_cost``
    per octave, one between voiced and unvoiced ``switch_cost``.  The defaults are Praat's path-finder settings (Boersma
    1993) moved to the scale of d'; they are not tuned on speech.  Float64 inside; the outputs never require grad."""
    B, F, K = _f0_path_shape("f0_viterbi", cand_period, cand_ap, sample_rate, lag_ref)
    if F < 1:
        raise _lib.GolfError(f"f0_viterbi: F={F} frames must be >= 1")
    if B * F >= 2 ** 31:
        raise _lib.GolfError(f"f0_viterbi: B*F = {B * F} frames, must be < 2^31")
    if B == 0:
        _lib.require_device(cand_period.float(), cand_ap.float())
        z = torch.empty(0, F, dtype=torch.float32, device=cand_period.device)
        return (z, torch.empty(0, F, dtype=torch.int32, device=cand_period.device)) if return_state else z
    return _f0_viterbi(cand_period, cand_ap, float(sample_rate), float(lag_ref), float(unvoiced_cost), float(lag_cost),
                       float(jump_cost), float(switch_cost), bool(return_state))


F0_STREAM_MAX_LAG = 1024   # csrc/f0_viterbi_stream.hip VS_MAX_LAG


def f0_viterbi_stream_decided(n: int, lag: int, flush: bool = False) -> int:
    """Frames of an utterance that are final once ``n`` of them have been consumed at ``lag``: all of them after a flush,
    ``max(n - lag, 0)`` before."""
    return n if flush else max(n - lag, 0)


def f0_viterbi_stream_state(B: int, K: int, lag: int, device) -> torch.Tensor:
    """The carry of ``f0_viterbi_stream`` for ``B`` rows of ``K`` candidates at ``lag`` frames: an opaque tensor that a call
    with ``f_done == 0`` need not find cleared."""
    B, K, lag = int(B), int(K), int(lag)
    if not 1 <= K <= F0_MAX_CANDIDATES:
        raise _lib.GolfError(f"f0_viterbi_stream: K={K} candidates must be 1..{F0_MAX_CANDIDATES}")
    if not 0 <= lag <= F0_STREAM_MAX_LAG:
        raise _lib.GolfError(f"f0_viterbi_stream: lag={lag} frames must be 0..{F0_STREAM_MAX_LAG}")
    if B < 1:
        raise _lib.GolfError(f"f0_viterbi_stream: B={B} rows must be >= 1")
    nbytes = _lib.load().golf_f0_viterbi_stream_state_bytes(B, K, lag)
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


@_amp_no_grad   # as the one-shot path: under autocast fp16 / bf16 candidates become fp32
def f0_viterbi_stream(cand_period: torch.Tensor, cand_ap: torch.Tensor, carry: torch.Tensor, f_done: int, lag: int,
                      sample_rate: float, lag_ref: float, unvoiced_cost: float = 0.3, lag_cost: float = 0.02,
                      jump_cost: float = 0.35, switch_cost: float = 0.14, flush: bool = False, return_state: bool = False):
    """``f0_viterbi`` block by block (the definition is in include/golf_amd.h): the candidates (B, nf, K) of frames
    ``[f_done, f_done + nf)`` -> ``f0 (B, n_out)``, or with ``return_state`` ``(f0, state)``, of the frames that became final:
    frame g is decided once frame ``g + lag`` has been consumed, from the best path that ends there, and ``flush`` ends the
    utterance and decides the rest.  ``n_out = decided(f_done + nf, flush) - decided(f_done)`` with
    ``f0_viterbi_stream_decided``; it may be 0.  The result depends on the candidates and ``lag`` alone, not on the cuts, and
    for ``lag >= F - 1`` it is ``f0_viterbi``'s.  ``carry`` comes from ``f0_viterbi_stream_state`` and is updated in place;
    ``f_done == 0`` starts an utterance.  The outputs never require grad."""
    B, nf, K = _f0_path_shape("f0_viterbi_stream", cand_period, cand_ap, sample_rate, lag_ref)
    f_done, lag, flush = int(f_done), int(lag), bool(flush)
    if not 0 <= lag <= F0_STREAM_MAX_LAG:
        raise _lib.GolfError(f"f0_viterbi_stream: lag={lag} frames must be 0..{F0_STREAM_MAX_LAG}")
    if f_done < 0:
        raise _lib.GolfError(f"f0_viterbi_stream: f_done={f_done} frames must be >= 0")
    if flush and f_done + nf < 1:
        raise _lib.GolfError("f0_viterbi_stream: F=0 frames must be >= 1 (a flush of an utterance of no frames)")
    if B * nf >= 2 ** 31 or f_done + nf >= 2 ** 31:
        raise _lib.GolfError(f"f0_viterbi_stream: B*F = {B * nf} and f_done + F = {f_done + nf} frames, must be < 2^31")
    if B < 1:
        raise _lib.GolfError(f"f0_viterbi_stream: B={B} rows must be >= 1")
    _lib.require_device(carry, dtype=torch.int64)
    _lib.require_device(cand_period, cand_ap)
    n_out = f0_viterbi_stream_decided(f_done + nf, lag, flush) - f0_viterbi_stream_decided(f_done, lag)
    dev = cand_period.device
    f0 = torch.empty(B, n_out, dtype=torch.float32, device=dev)
    state = torch.empty(B, n_out, dtype=torch.int32, device=dev) if return_state else None
    if nf > 0 or n_out > 0:   # nothing to consume and nothing to decide: nothing to launch
        lib = _lib.load()
        cand_period, cand_ap = cand_period.contiguous(), cand_ap.contiguous()
        rcode = lib.golf_f0_viterbi_stream_f32(cand_period.data_ptr(), cand_ap.data_ptr(), f0.data_ptr(), _lib.ptr(state),
                                               max(n_out, 1), carry.data_ptr(), carry.numel() * 8, B, nf, K, lag, f_done,
                                               int(flush), float(sample_rate), float(lag_ref), float(unvoiced_cost),
                                               float(lag_cost), float(jump_cost), float(switch_cost), _lib.stream_ptr())
        _lib.check(rcode, "golf_f0_viterbi_stream_f32")
    return (f0, state) if return_state else f0


def f0_track(x: torch.Tensor, sample_rate: float, hop: int, f0_min: float = 60.0, f0_max: float = 1000.0,
             window_length: int = None, n_candidates: int = 7, rms_floor: float = 0.0, centred: bool = True,
             n_frames: int = None, unvoiced_cost: float = 0.3, lag_cost: float = 0.02, jump_cost: float = 0.35,
             switch_cost: float = 0.14, return_all: bool = False):
    """f0 by ``f0_candidates`` and ``f0_viterbi`` with ``lag_ref = tau_min``: x (B, T) -> ``f0 (B, F)`` in Hz, 0 where the path
    is unvoiced, or with ``return_all`` ``(f0, state, cand_period, cand_ap)``.  Where ``f0_yin`` decides every frame on its
    own, this decides the utterance: an octave jump or a dropped frame costs more than it gains."""
    cand_period, cand_ap = f0_candidates(x, sample_rate, hop, f0_min, f0_max, window_length, n_candidates, rms_floor, centred,
                                         n_frames)
    tau_min = f0_lags(float(sample_rate), float(f0_min), float(f0_max), window_length)[0]
    out = f0_viterbi(cand_period, cand_ap, sample_rate, float(tau_min), unvoiced_cost, lag_cost, jump_cost, switch_cost,
                     return_state=return_all)
    return (out[0], out[1], cand_period, cand_ap) if return_all else out


# ------------------------------------------------------------------------------------------------
def ff_output_length(Tx: int, F: int, hop: int, W: int):
    """(Tx_used, nfr, Ty) of the frame-wise filter (reference models/filters.py:147-180)."""
    Tx = min(Tx, (F - 1) * hop + 1)
    pad = W // 2
    nfr = (Tx + 2 * pad - W) // hop + 1
    Ty = (nfr - 1) * hop + W - 2 * pad
    return Tx, nfr, Ty


# (ring width, largest order it serves) of the frame-wise filter's ring kernels (csrc/lpc_ff.hip GOLF_FF_TRY): the first ring
# with M <= order whose width fits into one hop.  Every other shape runs -- and trains -- on the wave-per-frame kernels of
# csrc/lpc_ff_any.hip.
FF_RINGS = SS_RINGS


def ff_on_ring_grid(M: int, hop: int, W: int = None, backward: bool = False) -> bool:
    """True when the frame-wise filter runs (lpc order, hop) -- for ``backward=True``: differentiates (lpc order, hop, window
    length W) -- on the ring kernels of csrc/lpc_ff.hip; False: the wave-per-frame kernels of csrc/lpc_ff_any.hip (any
    1 <= M <= 64, hop >= 1).  The forward has a ring kernel for every window; the backward's ring chain needs a window that
    is a multiple of the ring width, and short enough (about 2030 samples) for its g_a kernel to stage two whole frames per
    wave in LDS.  Restates the routing of golf_lti_frames_ola_{fwd,bwd}_f32 for tools and tests."""
    ring = next((ring for ring, order in FF_RINGS if M <= order and ring <= hop), None)
    if ring is None:
        return False
    if not backward:
        return True
    if W is None:
        raise ValueError("ff_on_ring_grid(backward=True) needs the window length")
    return W % ring == 0 and 16 * (2 * W + ring + 6) <= 64 * 1024


class _LTIFramesOLA(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, gain, a, window, hop):
        _lib.require_device(ex, gain, a, window)
        lib = _lib.load()
        ex = _rows(ex)
        gain = gain.contiguous()
        a = a.contiguous()
        window = window.contiguous()
        B, Tx0 = ex.shape
        F, M = a.shape[1], a.shape[2]
        W = window.numel()
        Tx, nfr, Ty = ff_output_length(Tx0, F, hop, W)
        if nfr > F:
            raise _lib.GolfError(f"frame-wise filter: {nfr} frames needed but only {F} coefficient frames")
        y = torch.empty(B, Ty, dtype=torch.float32, device=ex.device)
        ws = _workspace(lib.golf_lti_frames_workspace_bytes(B, Tx, F, M, hop, W), ex.device)
        rc = lib.golf_lti_frames_ola_fwd_f32(ex.data_ptr(), ex.stride(0), gain.data_ptr(), a.data_ptr(),
                                             window.data_ptr(), y.data_ptr(), y.stride(0), B, Tx, F, M, hop, W, Ty,
                                             ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "golf_lti_frames_ola_fwd_f32")
        ctx.save_for_backward(ex, gain, a, window, ws)  # ws holds the filtered frames the backward needs
        ctx.geom = (hop, Tx, Ty)
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        ex, gain, a, window, ws_fwd = ctx.saved_tensors
        hop, Tx, Ty = ctx.geom
        lib = _lib.load()
        gy = _rows(gy)
        B, Tx0 = ex.shape
        F, M = a.shape[1], a.shape[2]
        W = window.numel()
        g_ex = torch.empty(B, Tx0, dtype=torch.float32, device=ex.device)   # written in full by the backward (zeros in the tail)
        g_gain = torch.empty_like(gain)
        g_a = torch.empty_like(a)
        ws = _workspace(lib.golf_lti_frames_bwd_workspace_bytes(B, Tx, F, M, hop, W), ex.device)
        rc = lib.golf_lti_frames_ola_bwd_f32(gy.data_ptr(), gy.stride(0), ex.data_ptr(), ex.stride(0),
                                             gain.data_ptr(), a.data_ptr(), window.data_ptr(), g_ex.data_ptr(),
                                             g_ex.stride(0), Tx0, g_gain.data_ptr(), g_a.data_ptr(), B, Tx, F, M, hop,
                                             W, Ty, ws_fwd.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "golf_lti_frames_ola_bwd_f32")
        return g_ex, g_gain, g_a, None, None


def lti_frames_ola(ex, gain, a, window, hop: int) -> torch.Tensor:
    """Frame-wise LTI all-pole filter + windowed overlap-add (include/golf_amd.h a-4): ex (B, Tx), gain (B, F), a (B, F, M),
    window (W,), W even and >= 2*hop; differentiable w.r.t. ex, gain and a.  Any order 1 <= M <= 64 and any hop >= 1: the
    ring kernels where ``ff_on_ring_grid`` holds, one wave per frame elsewhere; M > 64 raises GolfError."""
    return _LTIFramesOLA.apply(ex, gain, a, window, int(hop))


def _ola_carry(nbytes: int, B: int, W: int, device) -> torch.Tensor:
    return torch.zeros(int(B), nbytes // (4 * int(B) * int(W)), int(W), dtype=torch.float32, device=device)


def _ola_stream_tail(who, carry, make_carry, geometry, nf, ny, device):
    """What the two overlap-add stream entries share once their inputs are checked: the carry (``make_carry(*geometry,
    device)`` when None, geometry = (B, W, ...)), the (B, ny) output and the (B, S + nf, W) workspace (None for an empty call)."""
    B, W = geometry[:2]
    if carry is None:
        carry = make_carry(*geometry, device)
    if not carry.is_cuda or carry.dtype != torch.float32 or not carry.is_contiguous() or carry.shape[0] != B:
        raise _lib.GolfError(f"{who}: carry {tuple(carry.shape)} {carry.dtype} (from {make_carry.__name__})")
    y = torch.empty(B, int(ny), dtype=torch.float32, device=device)
    ws = _workspace(4 * B * (carry.shape[1] + int(nf)) * W, device) if nf > 0 or ny > 0 else None
    return carry, y, ws


def lti_frames_stream_carry(B: int, W: int, hop: int, M: int, device) -> torch.Tensor:
    """The zeroed (B, ceil(W/hop) - 1, W) fp32 carry of ``lti_frames_ola_stream``: the last filtered frames."""
    nbytes = _lib.load().golf_lti_frames_stream_state_bytes(int(B), int(W), int(hop), int(M))
    if nbytes == 0:
        raise _lib.GolfError(f"lti_frames_ola_stream: no carry for B={B}, W={W}, hop={hop}, M={M} (W >= 2*hop, M <= 38)")
    return _ola_carry(nbytes, B, W, device)


def lti_frames_ola_stream(ex, gain, a, window, hop: int, carry=None, *, x0: int, g0: int, a0: int, f0: int, nf: int,
                          n0: int, ny: int, x_end: int = -1, g_end: int = -1):
    """One call of the frame-wise filter run block by block (golf_lti_frames_ola_stream_f32), global indices throughout:
    filters frames [f0, f0+nf) and returns output samples [n0, n0+ny) as a (B, ny) fp32 tensor, together with the carry
    (allocated when ``carry`` is None: pass None to the first call and the returned one to every later call).
    ``ex`` (B, nx) holds samples x0 .., ``gain`` (B, ng) rows g0 .., ``a`` (B, na, M) rows a0 ..; ``x_end`` / ``g_end``: the
    utterance's Tx and F once it has ended (-1 before).  Inference only; fp16 / bf16 tracks are cast to fp32 first."""
    _inference_only("lti_frames_ola_stream", ex, gain, a)
    ex, gain, a = _rows(ex.float()), gain.float().contiguous(), a.float().contiguous()
    window = window.float().contiguous()
    _lib.require_device(ex, gain, a, window)
    B, nx = ex.shape
    M, W = a.shape[2], window.numel()
    if gain.shape[0] != B or a.shape[0] != B or gain.ndim != 2:
        raise _lib.GolfError(f"lti_frames_ola_stream: ex {tuple(ex.shape)}, gain {tuple(gain.shape)}, a {tuple(a.shape)}")
    carry, y, ws = _ola_stream_tail("lti_frames_ola_stream", carry, lti_frames_stream_carry, (B, W, hop, M), nf, ny, ex.device)
    lib = _lib.load()
    rc = lib.golf_lti_frames_ola_stream_f32(ex.data_ptr(), ex.stride(0), int(x0), nx, int(x_end), gain.data_ptr(), int(g0),
                                            gain.shape[1], int(g_end), a.data_ptr(), int(a0), a.shape[1], window.data_ptr(),
                                            int(f0), int(nf), y.data_ptr(), y.stride(0), int(n0), int(ny), B, M, int(hop), W,
                                            carry.data_ptr(), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                            _lib.stream_ptr())
    _lib.check(rc, "golf_lti_frames_ola_stream_f32")
    return y, carry


def stft_filter_stream_carry(B: int, n_fft: int, hop: int, device) -> torch.Tensor:
    """The zeroed (B, ceil(n_fft/hop) - 1, n_fft) fp32 carry of ``stft_filter_stream``: the last filtered frames."""
    nbytes = _lib.load().golf_stft_filter_stream_state_bytes(int(B), int(n_fft), int(hop))
    if nbytes == 0:
        raise _lib.GolfError(f"stft_filter_stream: no carry for B={B}, n_fft={n_fft}, hop={hop} (n_fft a power of two in "
                             "[64, 2048], n_fft >= 2*hop)")
    return _ola_carry(nbytes, B, n_fft, device)


def stft_filter_stream(x, H, window, hop: int, carry=None, *, x0: int, h0: int, f0: int, nf: int, n0: int, ny: int,
                       x_end: int = -1, frames_end: int = -1):
    """One call of the STFT-domain frame filter run block by block (golf_stft_filter_frames_stream_f32), global indices
    throughout: filters frames [f0, f0+nf) and returns output samples [n0, n0+ny) as a (B, ny) fp32 tensor, together with
    the carry (allocated when ``carry`` is None: pass None to the first call and the returned one to every later call).
    ``x`` (B, nx) holds samples x0 ..; ``H`` (B, nh, n_fft/2+1), real or complex, holds the response rows h0 .. on bins
    0 .. n_fft/2; ``x_end`` / ``frames_end``: the utterance's length and frame count once it has ended (-1 before).
    Inference only; fp16 / bf16 tracks are cast to fp32 first."""
    _inference_only("stft_filter_stream", x, H)
    x, window = _rows(x.float()), window.float().contiguous()
    cplx = H.is_complex()
    Hf = torch.view_as_real(H.to(torch.complex64).contiguous()) if cplx else H.float().contiguous()
    _lib.require_device(x, Hf, window)
    B, nx = x.shape
    n = window.numel()
    if H.ndim != 3 or H.shape[0] != B or H.shape[2] != n // 2 + 1:
        raise _lib.GolfError(f"stft_filter_stream: x {tuple(x.shape)}, H {tuple(H.shape)}, n_fft {n}")
    carry, y, ws = _ola_stream_tail("stft_filter_stream", carry, stft_filter_stream_carry, (B, n, hop), nf, ny, x.device)
    lib = _lib.load()
    rc = lib.golf_stft_filter_frames_stream_f32(x.data_ptr(), x.stride(0), int(x0), nx, int(x_end), Hf.data_ptr(), int(h0),
                                                H.shape[1], int(cplx), int(frames_end), window.data_ptr(), int(f0), int(nf),
                                                y.data_ptr(), y.stride(0), int(n0), int(ny), B, n, int(hop),
                                                carry.data_ptr(), _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                                _lib.stream_ptr())
    _lib.check(rc, "golf_stft_filter_frames_stream_f32")
    return y, carry


class _STFTFilterFrames(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, H, window, hop):
        ctx.dtypes = (x.dtype, H.dtype)
        x, window = _rows(x.float()), window.float().contiguous()
        cplx = H.is_complex()
        H = H.to(torch.complex64).contiguous() if cplx else H.float().contiguous()
        T = x.shape[1]
        frames = min(1 + T // hop, H.shape[1])
        # the streaming entry in a single call: end markers set, a fresh zero carry
        y = stft_filter_stream(x, H, window, hop, None, x0=0, h0=0, f0=0, nf=frames, n0=0, ny=hop * (frames - 1), x_end=T,
                               frames_end=frames)[0]
        ctx.save_for_backward(x, torch.view_as_real(H) if cplx else H, window)
        ctx.hop = hop
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        x, Hf, window = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad[:2]
        lib = _lib.load()
        gy = _rows(gy)
        B, T = x.shape
        F, n = Hf.shape[1], window.numel()
        g_x = torch.empty(B, T, dtype=torch.float32, device=x.device) if need_x else None   # written in full
        g_h = torch.empty_like(Hf) if need_h else None                                     # (zeros for the rows no frame uses)
        ws = _workspace(lib.golf_stft_filter_frames_bwd_workspace_bytes(B, T, F, n, ctx.hop), x.device)
        rc = lib.golf_stft_filter_frames_bwd_f32(gy.data_ptr(), gy.stride(0), x.data_ptr(), x.stride(0), Hf.data_ptr(),
                                                 int(Hf.ndim == 4), window.data_ptr(), _lib.ptr(g_x),
                                                 T if g_x is None else g_x.stride(0), _lib.ptr(g_h), B, T, F, n, ctx.hop,
                                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "golf_stft_filter_frames_bwd_f32")
        if need_h:
            g_h = (torch.view_as_complex(g_h) if Hf.ndim == 4 else g_h).to(ctx.dtypes[1])
        return g_x.to(ctx.dtypes[0]) if need_x else None, g_h, None, None


def stft_filter_frames(x, H, window, hop: int) -> torch.Tensor:
    """The STFT-domain frame filter over a whole utterance: ``x`` (B, T), ``H`` (B, F, n_fft/2+1) real or complex -> (B,
    hop*(frames-1)), frames = min(1 + T//hop, F).  What LTVCepFilter / DiffWorldSPFilter compute with torch.stft / torch.istft,
    and what they run on the device.  The forward is ``stft_filter_stream`` in a single call with the end markers set;
    differentiable w.r.t. ``x`` and ``H`` (golf_stft_filter_frames_bwd_f32), the gradient of a complex ``H`` in torch's
    convention (d/d re + i d/d im)."""
    T, n = x.shape[1], window.numel()
    if T <= n // 2:
        raise _lib.GolfError(f"stft_filter_frames: {T} samples cannot be reflect-padded by n_fft/2 = {n // 2}")
    return _STFTFilterFrames.apply(x, H, window, int(hop))


# ------------------------------------------------------------------------------------------------
# mel-cepstral filter design: mel cepstra -> complex minimum-phase response rows (include/golf_amd.h, csrc/mlsa_design.hip)
# ------------------------------------------------------------------------------------------------
def mel_cepstrum_tables(n_fft: int, order: int, alpha: float, dtype=torch.float32, device=None):
    """cos(m theta_k) and sin(m theta_k), (order + 1, n_fft/2 + 1) each, evaluated in float64 and rounded to ``dtype``;
    theta_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k) is the all-pass phase warp of w_k = 2 pi k / n_fft.  The sine
    is exactly 0 at bins 0 and n_fft/2 (sin(m pi) is 1e-14 in float64), so that the response is real there."""
    w = 2.0 * math.pi * torch.arange(n_fft // 2 + 1, dtype=torch.float64, device=device) / n_fft
    theta = w + 2.0 * torch.atan2(alpha * torch.sin(w), 1.0 - alpha * torch.cos(w))
    angle = torch.arange(order + 1, dtype=torch.float64, device=device).unsqueeze(1) * theta
    c, s = torch.cos(angle), torch.sin(angle)
    s[:, 0] = s[:, -1] = 0
    return c.to(dtype), s.to(dtype)


def mel_cepstrum_response_torch(mc: torch.Tensor, n_fft: int, alpha: float, tables=None) -> torch.Tensor:
    """The definition of ``mel_cepstrum_response`` in plain torch, in ``mc``'s precision and on its device: two real
    contractions with ``mel_cepstrum_tables`` (built here unless passed), exp of the complex logarithm.  What CPU tensors,
    float64 and the geometries the kernel refuses run, and what the kernel is timed against."""
    c, s = tables if tables is not None else mel_cepstrum_tables(n_fft, mc.shape[-1] - 1, alpha, mc.dtype, mc.device)
    return torch.exp(torch.complex(mc @ c, -(mc @ s)))


def mel_cepstrum_kernel_takes(n_fft: int, order: int, alpha: float) -> bool:
    """Whether golf_mlsa_response_rows_f32 covers the geometry: n_fft a power of two in [64, 2048], order <= 64, |alpha| < 1."""
    return n_fft & (n_fft - 1) == 0 and 64 <= n_fft <= 2048 and 0 <= order <= 64 and -1.0 < alpha < 1.0


def mel_cepstrum_basis(n_fft: int, order: int, alpha: float, device) -> torch.Tensor:
    """The kernel's basis for (n_fft, order, alpha) on ``device`` (golf_mlsa_response_basis_f32), a flat fp32 tensor holding
    ``mel_cepstrum_tables`` with rows padded to n_fft/2 + 64.  Enqueued on the current stream; the caller owns it.  Raises
    ``GolfError`` for a geometry the kernel refuses."""
    if torch.device(device).type != "cuda":
        raise _lib.GolfError("golf_amd kernels need ROCm device tensors (mel_cepstrum_basis on %s); there is no CPU path"
                             % torch.device(device).type)
    lib = _lib.load()
    nbytes = lib.golf_mlsa_response_basis_bytes(int(n_fft), int(order))
    b = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device)   # never a null pointer: the entry names the reason
    with torch.cuda.device(b.device):
        _lib.check(lib.golf_mlsa_response_basis_f32(int(n_fft), int(order), float(alpha), b.data_ptr(), nbytes,
                                                    _lib.stream_ptr()), "golf_mlsa_response_basis_f32")
    return b


def mel_cepstrum_rows(mc: torch.Tensor, basis: torch.Tensor, n_fft: int) -> torch.Tensor:
    """(..., order + 1) fp32 mel cepstra on the device -> (..., n_fft/2 + 1) complex64 response rows
    (golf_mlsa_response_rows_f32; no autograd).  ``basis`` from ``mel_cepstrum_basis`` for the same n_fft and order."""
    _lib.require_device(mc, basis)
    mc = mc.detach().contiguous()
    h = torch.empty(*mc.shape[:-1], n_fft // 2 + 1, 2, dtype=torch.float32, device=mc.device)
    if mc.numel() == 0:   # an empty block of a stream: no rows, no launch (and no pointer to pass)
        return torch.view_as_complex(h)
    _lib.check(_lib.load().golf_mlsa_response_rows_f32(mc.data_ptr(), basis.data_ptr(), basis.numel() * 4, h.data_ptr(),
                                                       mc.numel() // mc.shape[-1], int(n_fft), mc.shape[-1] - 1,
                                                       _lib.stream_ptr()), "golf_mlsa_response_rows_f32")
    return torch.view_as_complex(h)


class _MelCepstrumRows(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, mc, basis, n_fft):
        h = mel_cepstrum_rows(mc, basis, n_fft)
        ctx.save_for_backward(mc.detach().contiguous(), basis)
        ctx.n_fft = n_fft
        return h

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_h):
        mc, basis = ctx.saved_tensors
        g = torch.view_as_real(g_h.resolve_conj().to(torch.complex64).contiguous())
        g_mc = torch.empty_like(mc)   # written in full
        if mc.numel() == 0:
            return g_mc, None, None
        _lib.check(_lib.load().golf_mlsa_response_rows_bwd_f32(g.data_ptr(), mc.data_ptr(), basis.data_ptr(), basis.numel() * 4,
                                                               g_mc.data_ptr(), mc.numel() // mc.shape[-1], ctx.n_fft,
                                                               mc.shape[-1] - 1, _lib.stream_ptr()),
                   "golf_mlsa_response_rows_bwd_f32")
        return g_mc, None, None


def mel_cepstrum_response(mc: torch.Tensor, n_fft: int, alpha: float, basis: torch.Tensor = None) -> torch.Tensor:
    """(..., M + 1) mel cepstra -> (..., n_fft/2 + 1) complex minimum-phase response rows H = exp(sum_m mc[m] e^{-j m theta_k})
    on the warped frequencies theta_k (include/golf_amd.h; gamma = 0).  fp32 tensors on a ROCm device -- fp16 / bf16 under
    autocast -- with a geometry the kernel takes (``mel_cepstrum_kernel_takes``) run golf_mlsa_response_rows_{,bwd_}f32:
    differentiable w.r.t. ``mc``, a row's bits independent of the other rows.  ``basis``: the ``mel_cepstrum_basis`` of
    (n_fft, M, alpha), built per call when None (a module keeps its own).  Everything else -- CPU tensors, float64, n_fft =
    1000, M > 64 -- is ``mel_cepstrum_response_torch``."""
    dtypes = (torch.float32, torch.float16, torch.bfloat16) if torch.is_autocast_enabled() else (torch.float32,)
    if not (mc.is_cuda and mc.dtype in dtypes and mel_cepstrum_kernel_takes(int(n_fft), mc.shape[-1] - 1, float(alpha))):
        return mel_cepstrum_response_torch(mc, int(n_fft), float(alpha))
    if basis is None:
        basis = mel_cepstrum_basis(n_fft, mc.shape[-1] - 1, alpha, mc.device)
    return _MelCepstrumRows.apply(mc, basis, int(n_fft))


# ------------------------------------------------------------------------------------------------
# control transform of the LPC filters: logits -> direct-form coefficients (reference models/utils.py:581-593)
# ------------------------------------------------------------------------------------------------
class _RC2LPC(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, logits, max_abs, apply_tanh):
        _lib.require_device(logits)
        lib = _lib.load()
        x = logits.float().contiguous()
        M = x.shape[-1]
        N = x.numel() // M
        a = torch.empty_like(x)
        _lib.check(lib.golf_rc2lpc_fwd_f32(x.data_ptr(), a.data_ptr(), N, M, float(max_abs), int(apply_tanh),
                                           _lib.stream_ptr()), "golf_rc2lpc_fwd_f32")
        ctx.cfg = (float(max_abs), int(apply_tanh))
        ctx.save_for_backward(x)
        return a

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_a):
        (x,) = ctx.saved_tensors
        max_abs, apply_tanh = ctx.cfg
        lib = _lib.load()
        M = x.shape[-1]
        g = g_a.float().contiguous()
        out = torch.empty_like(x)
        _lib.check(lib.golf_rc2lpc_bwd_f32(x.data_ptr(), g.data_ptr(), out.data_ptr(), x.numel() // M, M, max_abs,
                                           apply_tanh, _lib.stream_ptr()), "golf_rc2lpc_bwd_f32")
        return out, None, None


def rc2lpc_logits(logits: torch.Tensor, max_abs: float = 1.0) -> torch.Tensor:
    """``rc2lpc(tanh(logits) * max_abs)`` (..., M) -> (..., M) as ONE kernel (forward and backward)."""
    return _RC2LPC.apply(logits, float(max_abs), True)


def rc2lpc(rc: torch.Tensor) -> torch.Tensor:
    """Levinson step-up of given reflection coefficients (..., M) -> a_1..a_M, one kernel, differentiable."""
    return _RC2LPC.apply(rc, 1.0, False)


_SOS_REP = {"coef": 0, "conj": 1, "real": 2}


class _SOS2LPC(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, logits, max_abs_pole, rep):
        _lib.require_device(logits)
        lib = _lib.load()
        x = logits.float().contiguous()
        M = x.shape[-1]
        assert M % 2 == 0, "two logits per second-order section"
        N = x.numel() // M
        a = torch.empty_like(x)
        _lib.check(lib.golf_sos2lpc_fwd_f32(x.data_ptr(), a.data_ptr(), N, M // 2, float(max_abs_pole), int(rep),
                                            _lib.stream_ptr()), "golf_sos2lpc_fwd_f32")
        ctx.cfg = (float(max_abs_pole), int(rep))
        ctx.save_for_backward(x)
        return a

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_a):
        (x,) = ctx.saved_tensors
        rho, rep = ctx.cfg
        lib = _lib.load()
        M = x.shape[-1]
        g = g_a.float().contiguous()
        out = torch.empty_like(x)
        _lib.check(lib.golf_sos2lpc_bwd_f32(x.data_ptr(), g.data_ptr(), out.data_ptr(), x.numel() // M, M // 2, rho, rep,
                                            _lib.stream_ptr()), "golf_sos2lpc_bwd_f32")
        return out, None, None


def biquad_logits2lpc(logits: torch.Tensor, rep_type: str, max_abs_pole: float = 0.99) -> torch.Tensor:
    """``biquads2lpc(get_logits2biquads(rep_type, max_abs_pole)(logits.view(..., K, 2)))`` (..., 2K) -> (..., 2K) as
    ONE kernel, forward and backward."""
    return _SOS2LPC.apply(logits, float(max_abs_pole), _SOS_REP[rep_type])


# ------------------------------------------------------------------------------------------------
def osc_lengths(Tp: int, phase_hop: int, os: int):
    """(N oversampled length, Tout)."""
    P = phase_hop * os
    N = (Tp - 1) * P + 1 if P > 1 else Tp
    Tout = (N - 1) // os + 1 if os > 1 else N
    return N, Tout


_TAP_FRAGS: dict = {}   # (taps pointer, version, K, os, device) -> the taps' Toeplitz fragments (golf_glottal_osc_tap_fragments_f32)


def osc_tap_fragments(taps: torch.Tensor, os: int):
    """The decimation taps laid out for the matrix pipe, prepared once per tap set (ABI 6; the module's taps are a constant
    buffer, so this runs once per module and device).  None where the fused oscillator does not apply, and -- so that no
    allocation of a graph's private pool ends up in a process-wide cache -- when asked for the first time during a hipGraph
    capture: the library then lays them out inside the call, as it did every step until round 5."""
    if taps is None or taps.numel() == 0:
        return None
    key = (taps.data_ptr(), taps._version, taps.numel(), int(os), taps.device)
    hit = _TAP_FRAGS.get(key)
    if hit is not None:
        return hit[0]
    lib = _lib.load()
    n = lib.golf_glottal_osc_tap_fragments_bytes(taps.numel(), int(os))
    if n == 0 or torch.cuda.is_current_stream_capturing():
        return None
    frags = torch.empty(n, dtype=torch.uint8, device=taps.device)
    _lib.check(lib.golf_glottal_osc_tap_fragments_f32(taps.data_ptr(), taps.numel(), int(os), frags.data_ptr(), n,
                                                      _lib.stream_ptr()), "golf_glottal_osc_tap_fragments_f32")
    if len(_TAP_FRAGS) >= 16:
        _TAP_FRAGS.pop(next(iter(_TAP_FRAGS)))
    _TAP_FRAGS[key] = (frags, taps)   # (the taps tensor is kept alive with its fragments: the key is its address)
    return frags


class _GlottalOsc(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, phase, wsel, table, taps, phase_hop, w_hop, os, equal_energy, want_pre, add=None):
        _lib.require_device(phase, wsel, table, taps)
        if add is not None:
            assert os > 1 and add.ndim == 2 and add.shape[0] == phase.shape[0]
            _lib.require_device(add)
            add = _rows(add.float())
        if phase.requires_grad or table.requires_grad:
            raise NotImplementedError("golf_amd: the FUSED glottal oscillator differentiates w.r.t. table_select_weight "
                                      "only; use functional.wavetable_osc (IndexedGlottalFlowTable does so on its own) "
                                      "for gradients w.r.t. phase / the table")
        lib = _lib.load()
        phase = _rows(phase)
        wsel = wsel.contiguous()
        table = table.contiguous()
        B, Tp = phase.shape
        Fw = wsel.shape[1]
        n_tab, L = table.shape
        K = 0 if taps is None else taps.numel()
        if os > 1:
            assert taps is not None and K % 2 == 1, "decimation taps (odd length) required when oversampling > 1"
            taps = taps.contiguous()
        N, Tout = osc_lengths(Tp, phase_hop, os)
        out = torch.empty(B, Tout, dtype=torch.float32, device=phase.device)
        pre = torch.empty(B, N, dtype=torch.float32, device=phase.device) if (want_pre and os > 1) else None
        ws = _workspace(lib.golf_glottal_osc_workspace_bytes(B, Tp, phase_hop, Fw, w_hop, L, os), phase.device)
        frags = osc_tap_fragments(taps, os) if (os > 1 and not want_pre) else None
        rc = lib.golf_glottal_osc_fwd_f32(phase.data_ptr(), phase.stride(0), Tp, phase_hop, wsel.data_ptr(), Fw, w_hop,
                                          table.data_ptr(), n_tab, L, os,
                                          int(bool(equal_energy)) | (OSC_THROUGHPUT if THROUGHPUT_MODE else 0), _lib.ptr(taps), K,
                                          _lib.ptr(pre), out.data_ptr(), out.stride(0), B, Tout, ws.data_ptr(),
                                          ws.numel(), _lib.stream_ptr(), _lib.ptr(add),
                                          0 if add is None else add.stride(0), 0 if add is None else add.shape[1],
                                          _lib.ptr(frags))
        _lib.check(rc, "golf_glottal_osc_fwd_f32")
        ctx.frags = frags   # a backward that reuses the workspace takes the fragments its forward took
        ctx.cfg = (phase_hop, w_hop, os, bool(equal_energy))
        ctx.ws_kept = pre is None   # the saved workspace is private to this node: the backward may reuse the forward's totals
        ctx.add_len = None if add is None else add.shape[1]
        ctx.save_for_backward(phase, wsel, table, taps if taps is not None else phase.new_empty(0), ws)
        ctx.mark_non_differentiable(*([pre] if pre is not None else []))
        return (out, pre) if pre is not None else (out, None)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_out, _g_pre):
        phase, wsel, table, taps, ws = ctx.saved_tensors
        phase_hop, w_hop, os, eq = ctx.cfg
        lib = _lib.load()
        B, Tp = phase.shape
        Fw = wsel.shape[1]
        n_tab, L = table.shape
        K = taps.numel()
        g_out = _rows(g_out.float())
        g_w = torch.empty_like(wsel)
        rc = lib.golf_glottal_osc_bwd_wsel_f32(g_out.data_ptr(), g_out.stride(0), phase.data_ptr(), phase.stride(0), Tp,
                                               phase_hop, wsel.data_ptr(), Fw, w_hop, table.data_ptr(), n_tab, L, os,
                                               int(eq) | (OSC_WS_KEPT if ctx.ws_kept else 0), _lib.ptr(taps) if K else 0, K,
                                               g_w.data_ptr(), B,
                                               g_out.shape[1], ws.data_ptr(), ws.numel(), _lib.stream_ptr(),
                                               _lib.ptr(ctx.frags))
        _lib.check(rc, "golf_glottal_osc_bwd_wsel_f32")
        g_add = None
        if ctx.add_len is not None and ctx.needs_input_grad[9]:   # out[:, :Tadd] += add
            n = min(ctx.add_len, g_out.shape[1])
            g_add = g_out[:, :n] if n == ctx.add_len else torch.nn.functional.pad(g_out, (0, ctx.add_len - n))
        return None, g_w, None, None, None, None, None, None, None, g_add


def glottal_osc(phase, wsel, table, taps, phase_hop: int, w_hop: int, oversampling: int = 1,
                equal_energy: bool = False, return_pre: bool = False, add=None):
    """Indexed glottal-flow wavetable oscillator (see include/golf_amd.h golf_glottal_osc_fwd_f32).
    ``add`` (B, Tadd), oversampling > 1: fused ``out[:, :Tadd] += add`` (differentiable w.r.t. ``add``); the caller
    truncates to the common length as AudioTensor addition would."""
    if phase.dim() == 2 and phase.shape[0] == 0:   # an empty batch: empty outputs of the right widths, like the reference's ops
        _lib.require_device(phase, wsel, table)
        N, Tout = osc_lengths(phase.shape[1], int(phase_hop), int(oversampling))
        out = phase.new_zeros(0, Tout) + 0.0 * wsel.sum()
        return (out, phase.new_zeros(0, N)) if return_pre else out
    if add is not None and oversampling <= 1:   # no decimator to fuse into
        out, pre = _GlottalOsc.apply(phase, wsel, table, taps, int(phase_hop), int(w_hop), int(oversampling),
                                     bool(equal_energy), bool(return_pre))
        n = min(out.shape[1], add.shape[1])
        out = torch.cat([out[:, :n] + add[:, :n], out[:, n:]], 1)
        return (out, pre) if return_pre else out
    out, pre = _GlottalOsc.apply(phase, wsel, table, taps, int(phase_hop), int(w_hop), int(oversampling),
                                 bool(equal_energy), bool(return_pre), add)
    return (out, pre) if return_pre else out


def source_filter_ss(phase, wsel, table, taps, phase_hop: int, w_hop: int, oversampling: int, equal_energy: bool,
                     gain, a, hop: int, add=None, mode: str = None, status: torch.Tensor = None,
                     length: int = None) -> torch.Tensor:
    """``ltv_allpole_ss(glottal_osc(phase, wsel, table, taps, ..., add=add), gain, a, hop)`` -- the decoder's source into its end
    filter (reference: SourceFilterSynth.forward, models/sf.py:47-64) -- with the oscillator and the filter's chunk transition
    maps in ONE launch (include/golf_amd.h golf_source_transitions_f32, ABI 6): the maps need only ``a``, and for a lone batch
    they are the long pole of the chain (38 us of issue-bound waves on 160 of 256 CUs, which the oscillator's workgroups fill).
    Inference only and bit-identical to the composition; whenever a gradient is required, or the shapes fall outside the fused
    launch, this IS the composition.  ``length``: as ``ltv_allpole_ss(..., length=)`` -- filter only the first ``length`` samples of
    the source (the decoder's common length of oscillator and filtered noise)."""
    ts = (phase, wsel, table, gain, a) + ((add,) if add is not None else ())
    if (torch.is_grad_enabled() and any(t.requires_grad for t in ts)) or oversampling <= 1 or phase.dim() != 2 or phase.shape[0] == 0:
        src = glottal_osc(phase, wsel, table, taps, phase_hop, w_hop, oversampling, equal_energy, add=add)
        return ltv_allpole_ss(src, gain, a, hop, mode=mode, status=status, length=length)
    _lib.require_device(phase, wsel, table, taps, gain, a)
    lib = _lib.load()
    phase, wsel, table, taps = _rows(phase.float()), wsel.float().contiguous(), table.float().contiguous(), taps.float().contiguous()
    gain, a = gain.float().contiguous(), a.float().contiguous()
    if add is not None:
        _lib.require_device(add)
        add = _rows(add.float())
    B, Tp = phase.shape
    Fw = wsel.shape[1]
    n_tab, L = table.shape
    K = taps.numel()
    os_ = int(oversampling)
    _, Tout = osc_lengths(Tp, int(phase_hop), os_)
    F, M = a.shape[1], a.shape[2]
    T = ss_output_length(Tout, F, int(hop))
    if length is not None:
        T = min(T, int(length))
        if T < 1:
            raise _lib.GolfError(f"source_filter_ss: length={length} leaves nothing to filter")
    flags = SS_MODES[mode] | FAST_TRANSITIONS | MAPS_ONLY
    src = torch.empty(B, Tout, dtype=torch.float32, device=phase.device)
    osc_ws = _workspace(lib.golf_glottal_osc_workspace_bytes(B, Tp, int(phase_hop), Fw, int(w_hop), L, os_), phase.device)
    ss_ws = _workspace(lib.golf_ltv_allpole_workspace_bytes_ex(B, T, F, M, int(hop), flags), phase.device)
    frags = osc_tap_fragments(taps, os_)
    rc = lib.golf_source_transitions_f32(phase.data_ptr(), phase.stride(0), Tp, int(phase_hop), wsel.data_ptr(), Fw, int(w_hop),
                                         table.data_ptr(), n_tab, L, os_, int(bool(equal_energy)), taps.data_ptr(), K,
                                         src.data_ptr(), src.stride(0), B, Tout, osc_ws.data_ptr(), osc_ws.numel(),
                                         _lib.ptr(add), 0 if add is None else add.stride(0), 0 if add is None else add.shape[1],
                                         _lib.ptr(frags), a.data_ptr(), T, F, M, int(hop), ss_ws.data_ptr(), ss_ws.numel(), flags,
                                         _lib.stream_ptr())
    _lib.check(rc, "golf_source_transitions_f32")
    handle = PreparedTransitions(ss_ws, (B, T, F, M, int(hop), a.data_ptr(), a._version, SS_MODES[mode]), None, a, True, False, True)
    with torch.no_grad():
        return ltv_allpole_ss(src, gain, a, hop, prepared=handle, fast_inference=True, mode=mode, status=status, length=length)


def glottal_osc_stream(phase, j0: int, nseg: int, final_point: bool, phase_hop: int, oversampling: int, wsel, w_first: int,
                       w_hop: int, table, equal_energy: bool, acc: torch.Tensor, want_wrapped: bool = False):
    """Fine-rate glottal oscillator samples of coarse phase samples j0 .. j0+nseg-1 (+ the utterance's last point with
    ``final_point``) from the carried Q0.64 phase ``acc`` ((B,) int64 holding the uint64 bits, updated in place):
    golf_glottal_osc_stream_f32.  ``phase`` (B, >= nseg+1) holds p[j0 ..], ``wsel`` (B, nw) rows w_first .. of the table-select
    track.  Returns (B, nseg*P + final_point) before decimation, and the wrapped phase at the same samples with
    ``want_wrapped`` (bit-identical to instantaneous_phase's).  Inference only."""
    _inference_only("glottal_osc_stream", phase, wsel, table)
    phase, wsel, table = _rows(phase.float()), _rows(wsel.float()), table.float().contiguous()
    _lib.require_device(phase, wsel, table)
    if not acc.is_cuda or acc.dtype != torch.int64 or acc.shape != (phase.shape[0],):
        raise _lib.GolfError(f"glottal_osc_stream: acc must be a ({phase.shape[0]},) int64 device tensor")
    B = phase.shape[0]
    P = int(phase_hop) * int(oversampling)
    n = int(nseg) * P + int(bool(final_point))
    pre = torch.empty(B, n, dtype=torch.float32, device=phase.device)
    wrapped = torch.empty_like(pre) if want_wrapped else None
    n_tab, L = table.shape
    lib = _lib.load()
    rc = lib.golf_glottal_osc_stream_f32(phase.data_ptr(), phase.stride(0), int(nseg), int(bool(final_point)), int(phase_hop),
                                         int(oversampling), wsel.data_ptr(), wsel.stride(0), wsel.shape[1], int(w_first),
                                         int(w_hop), table.data_ptr(), n_tab, L, int(bool(equal_energy)), int(j0),
                                         acc.data_ptr(), pre.data_ptr(), pre.stride(0), _lib.ptr(wrapped), B,
                                         _lib.stream_ptr())
    _lib.check(rc, "golf_glottal_osc_stream_f32")
    return (pre, wrapped) if want_wrapped else pre


# ------------------------------------------------------------------------------------------------
# generic (fully differentiable) table oscillator: wrapped phase -> bilinear table lookup (-> decimation)
# ------------------------------------------------------------------------------------------------
class _WavetableLookup(torch.autograd.Function):
    """GlottalFlowTable.generate (reference models/synth.py:124-177) on golf_wavetable_lookup_{fwd,bwd}_f32:
    out[b,n] = bilerp(tables[b], row n/hop_t, column wrapped[b,n]*L); differentiable w.r.t. both inputs."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, wrapped, tables, hop_t):
        _lib.require_device(wrapped, tables)
        lib = _lib.load()
        wrapped = _rows(wrapped)
        tables = tables.contiguous()
        B, N = wrapped.shape
        assert tables.ndim == 3 and tables.shape[0] == B
        K, L = tables.shape[1], tables.shape[2]
        out = torch.empty(B, N, dtype=torch.float32, device=wrapped.device)
        rc = lib.golf_wavetable_lookup_fwd_f32(wrapped.data_ptr(), wrapped.stride(0), tables.data_ptr(), K, L, hop_t,
                                               out.data_ptr(), out.stride(0), B, N, _lib.stream_ptr())
        _lib.check(rc, "golf_wavetable_lookup_fwd_f32")
        ctx.hop_t = hop_t
        ctx.save_for_backward(wrapped, tables)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_out):
        wrapped, tables = ctx.saved_tensors
        lib = _lib.load()
        B, N = wrapped.shape
        K, L = tables.shape[1], tables.shape[2]
        g_out = _rows(g_out.float())
        g_w = torch.empty_like(wrapped) if ctx.needs_input_grad[0] else None
        g_t = torch.empty_like(tables) if ctx.needs_input_grad[1] else None
        rc = lib.golf_wavetable_lookup_bwd_f32(g_out.data_ptr(), g_out.stride(0), wrapped.data_ptr(), wrapped.stride(0),
                                               tables.data_ptr(), K, L, ctx.hop_t, _lib.ptr(g_w),
                                               0 if g_w is None else g_w.stride(0), _lib.ptr(g_t), B, N,
                                               _lib.stream_ptr())
        _lib.check(rc, "golf_wavetable_lookup_bwd_f32")
        return g_w, g_t, None


def wavetable_lookup(wrapped: torch.Tensor, tables: torch.Tensor, hop_t: int) -> torch.Tensor:
    """wrapped (B,N) in [0,1], tables (B,K,L) at hop ``hop_t`` (frames beyond K-1 replicate the last) -> (B,N)."""
    return _WavetableLookup.apply(wrapped, tables, int(hop_t))


class _DecimateFIR(torch.autograd.Function):
    """The oscillator's decimator on its own (golf_decimate_fir_f32 / its adjoint)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, taps, os):
        _lib.require_device(x, taps)
        lib = _lib.load()
        x = _rows(x)
        taps = taps.contiguous()
        B, N = x.shape
        Tout = (N - 1) // os + 1
        out = torch.empty(B, Tout, dtype=torch.float32, device=x.device)
        rc = lib.golf_decimate_fir_f32(x.data_ptr(), x.stride(0), N, taps.data_ptr(), taps.numel(), os, out.data_ptr(),
                                       out.stride(0), B, Tout, _lib.stream_ptr())
        _lib.check(rc, "golf_decimate_fir_f32")
        ctx.cfg = (N, os)
        ctx.save_for_backward(taps)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_out):
        (taps,) = ctx.saved_tensors
        N, os = ctx.cfg
        lib = _lib.load()
        g_out = _rows(g_out.float())
        B, Tout = g_out.shape
        g_x = torch.empty(B, N, dtype=torch.float32, device=g_out.device)
        rc = lib.golf_decimate_fir_adj_f32(g_out.data_ptr(), g_out.stride(0), Tout, taps.data_ptr(), taps.numel(), os,
                                           g_x.data_ptr(), N, B, _lib.stream_ptr())
        _lib.check(rc, "golf_decimate_fir_adj_f32")
        return g_x, None, None


def decimate_fir(x: torch.Tensor, taps: torch.Tensor, os: int) -> torch.Tensor:
    return _DecimateFIR.apply(x, taps, int(os))


def linear_upsample(z: torch.Tensor, hop: int) -> torch.Tensor:
    """AudioTensor.reduce_hop_length on a plain (B,F) tensor (models/utils.py:171-191, 538-544)."""
    if hop == 1 or z.shape[1] == 1:
        return z
    n = (z.shape[1] - 1) * hop + 1
    return torch.nn.functional.interpolate(z[:, None], n, mode="linear", align_corners=True)[:, 0]


class _PhaseAccumulate(torch.autograd.Function):
    """wrapped = frac(cumsum(up(phase / os)) + offset) on the device (golf_phase_accumulate_f32: the exact 64-bit fixed-point
    prefix of the fused oscillator).  Backward: d wrapped / d inst = 1, so g_phase = up^T(reverse cumsum(g)) / os and
    g_offset = g -- what autograd does through cumsum and F.interpolate in the reference (models/synth.py:239-255)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, phase, phase_offset, phase_hop, os):
        # float64 / half phases are accepted like the tensor-op version did (the reference forces .float() here,
        # models/synth.py:251): cast first, then the fp32 / device contract applies
        off_meta = None if phase_offset is None else (phase_offset.shape, phase_offset.dtype)
        phase = _rows(phase.float())
        if phase_offset is not None:
            phase_offset = _rows(phase_offset.float().reshape(phase.shape[0], -1))
        _lib.require_device(phase, phase_offset)
        lib = _lib.load()
        B, Tp = phase.shape
        P = phase_hop * os
        N = (Tp - 1) * P + 1 if P > 1 else Tp
        if phase_offset is not None:   # AudioTensor addition truncates to the shorter operand (utils.py:230-232)
            N = min(N, phase_offset.shape[1])
        out = torch.empty(B, N, dtype=torch.float32, device=phase.device)
        ws = _workspace(lib.golf_phase_accumulate_workspace_bytes(B, Tp), phase.device)
        rc = lib.golf_phase_accumulate_f32(phase.data_ptr(), phase.stride(0), Tp, phase_hop, os, _lib.ptr(phase_offset),
                                           0 if phase_offset is None else phase_offset.stride(0), out.data_ptr(),
                                           out.stride(0), B, N, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "golf_phase_accumulate_f32")
        ctx.geom = (Tp, P, os, N, phase_offset is not None and phase_offset.shape[1])
        ctx.off_meta = off_meta
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        Tp, P, os, N, off_len = ctx.geom
        g_phase = g_off = None
        if ctx.needs_input_grad[0]:
            g_up = torch.flip(torch.cumsum(torch.flip(g.double(), [1]), 1), [1]).float()
            g_phase = upsample_adjoint(g_up, P, Tp) / os
        if ctx.needs_input_grad[1]:
            g_off = g.new_zeros(g.shape[0], off_len)
            g_off[:, :N] = g
            g_off = g_off.reshape(ctx.off_meta[0]).to(ctx.off_meta[1])   # the caller's shape and dtype
        return g_phase, g_off, None, None


def instantaneous_phase(phase: torch.Tensor, phase_hop: int, oversampling: int = 1, phase_offset: torch.Tensor = None):
    """(wrapped phase (B,N) float32 in [0,1], per-sample increment (B,N)): phase/os upsampled to the (oversampled) sample
    rate and accumulated exactly on the device (the reference: float32 cumsum, models/synth.py:250-251) plus the optional
    offset, wrapped; differentiable w.r.t. phase and phase_offset (custom backward: reverse cumulative sum + transposed
    upsampling, as in the reference).  The increment is a plain linear upsampling (it only scales the equal-energy factor)."""
    wrapped = _PhaseAccumulate.apply(phase, phase_offset, int(phase_hop), int(oversampling))
    ph = phase / oversampling if oversampling > 1 else phase
    up = linear_upsample(ph, phase_hop * oversampling)[:, : wrapped.shape[1]]
    return wrapped, up


def wavetable_osc(phase: torch.Tensor, phase_hop: int, tables: torch.Tensor, table_hop: int, oversampling: int = 1,
                  equal_energy: bool = False, phase_offset: torch.Tensor = None, taps: torch.Tensor = None,
                  decimate: bool = True) -> torch.Tensor:
    """The table oscillators of the reference in their general, fully differentiable form (models/synth.py:213-294):
    per-frame tables (B,K,L) at ``table_hop`` looked up at the running phase.  Differentiable w.r.t. ``phase``,
    ``tables`` and ``phase_offset``.  IndexedGlottalFlowTable routes here when anything but table_select_weight needs a
    gradient; the forward-only / weight-gradient case stays on the fused kernel (glottal_osc).
    ``decimate=False`` returns the oversampled signal."""
    wrapped, up = instantaneous_phase(phase, phase_hop, oversampling, phase_offset)
    v = wavetable_lookup(wrapped, tables, table_hop * oversampling)
    if equal_energy:
        v = v * torch.rsqrt(up)
    if oversampling > 1 and decimate:
        assert taps is not None, "decimation taps required when oversampling > 1"
        v = decimate_fir(v, taps, oversampling)
    return v


def blend_tables(table: torch.Tensor, wsel: torch.Tensor) -> torch.Tensor:
    """Two-row table blend of IndexedGlottalFlowTable (models/synth.py:223-237): (n_tab,L), (B,Fw) -> (B,Fw,L)."""
    n_tab = table.shape[0]
    idx = wsel * (n_tab - 1)
    i0 = idx.detach().long().clip_(0, n_tab - 2)
    p = (idx - i0).unsqueeze(-1)
    return table[i0] * (1 - p) + table[i0 + 1] * p


# ------------------------------------------------------------------------------------------------
# filtered-noise-band generator (reference models/noise.py:114-124)
# ------------------------------------------------------------------------------------------------
class _NoiseBand(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, log_gain, bands, offsets, hop, T):
        _lib.require_device(log_gain, bands)
        lib = _lib.load()
        log_gain, bands = log_gain.contiguous(), bands.contiguous()
        offsets = offsets.to(torch.int32).contiguous()
        B, F, K = log_gain.shape
        assert bands.shape[0] == K and offsets.shape == (B, K) and offsets.is_cuda
        Tout = min(T, (F - 1) * hop + 1) if F > 1 else T
        out = torch.empty(B, Tout, dtype=torch.float32, device=log_gain.device)
        rc = lib.golf_noise_band_fwd_f32(bands.data_ptr(), bands.shape[1], offsets.data_ptr(), log_gain.data_ptr(), F,
                                         hop, out.data_ptr(), out.stride(0), B, Tout, K, _lib.stream_ptr())
        _lib.check(rc, "golf_noise_band_fwd_f32")
        ctx.hop = hop
        ctx.save_for_backward(log_gain, bands, offsets)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_out):
        log_gain, bands, offsets = ctx.saved_tensors
        lib = _lib.load()
        B, F, K = log_gain.shape
        g_out = _rows(g_out.float())
        g_lg = torch.empty_like(log_gain)
        ws = _workspace(lib.golf_noise_band_workspace_bytes(B, F, K), log_gain.device)
        rc = lib.golf_noise_band_bwd_f32(g_out.data_ptr(), g_out.stride(0), bands.data_ptr(), bands.shape[1],
                                         offsets.data_ptr(), log_gain.data_ptr(), F, ctx.hop, g_lg.data_ptr(), B,
                                         g_out.shape[1], K, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "golf_noise_band_bwd_f32")
        return g_lg, None, None, None, None


def noise_band(bands: torch.Tensor, offsets: torch.Tensor, log_gain: torch.Tensor, hop: int, T: int) -> torch.Tensor:
    """bands (K, L) loopable noise periods, offsets (B,K) start indices, log_gain (B,F,K) at ``hop`` ->
    (B, min(T, (F-1)*hop+1)); differentiable w.r.t. log_gain (include/golf_amd.h golf_noise_band_*)."""
    return _NoiseBand.apply(log_gain, bands, offsets, int(hop), int(T))


# ------------------------------------------------------------------------------------------------
# LTV FIR filters designed from log magnitudes: zero-phase (the noise filter, reference models/filters.py:286-384) and
# minimum-phase (its causal twin, reference models/filters.py:198-283).  One code path; what differs is in _FIRDesign.
# ------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class _FIRDesign:
    """What tells the two designs apart: the name used in messages and cache keys, whether the frame filter that applies
    the kernels is causal, and the C entry points of the design (include/golf_amd.h)."""
    kind: str
    causal: bool
    basis_bytes: str
    basis: str
    kernels: str
    kernels_bwd: str


ZERO_PHASE_FIR = _FIRDesign("zero_phase", False, "golf_zero_phase_fir_basis_bytes", "golf_zero_phase_fir_basis_f32",
                            "golf_zero_phase_fir_kernels_f32", "golf_zero_phase_fir_kernels_bwd_f32")
MIN_PHASE_FIR = _FIRDesign("min_phase", True, "golf_min_phase_fir_basis_bytes", "golf_min_phase_fir_basis_f32",
                           "golf_min_phase_fir_kernels_f32", "golf_min_phase_fir_kernels_bwd_f32")

_basis_cache = {}


def _fir_basis(design: _FIRDesign, n_mag: int, device) -> torch.Tensor:
    dev = torch.device(device)
    key = (design.kind, n_mag, dev.index if dev.index is not None else torch.cuda.current_device())
    b = _basis_cache.get(key)
    if b is None:
        lib = _lib.load()
        nbytes = getattr(lib, design.basis_bytes)(n_mag)
        b = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        _lib.check(getattr(lib, design.basis)(n_mag, b.data_ptr(), nbytes, _lib.stream_ptr()), design.basis)
        _basis_cache[key] = b
    return b


def zero_phase_fir_basis(n_mag: int, device) -> torch.Tensor:
    """The constant cosine-transform matrix for ``n_mag`` bins (both orientations), built once per device."""
    return _fir_basis(ZERO_PHASE_FIR, n_mag, device)


def min_phase_fir_basis(n_mag: int, device) -> torch.Tensor:
    """The constant matrices of the minimum-phase design for ``n_mag`` bins (Hilbert transform on the half spectrum,
    cosine and sine synthesis, both orientations), built once per device."""
    return _fir_basis(MIN_PHASE_FIR, n_mag, device)


def min_phase_window(window_fn, n: int, device=None) -> torch.Tensor:
    """The reference's ``windowing`` (models/filters.py:216-221) as a vector: window_fn(n) with its first n // 2 entries
    set to 1 (the minimum-phase response starts at tap 0: only its tail is tapered)."""
    w = window_fn(n).to(dtype=torch.float32).clone()
    w[: n // 2] = 1
    return w.to(device=device).contiguous()


def _fir_kernels_raw(design: _FIRDesign, log_mag, window, basis):
    """Contiguous device tensors log_mag (B,F,n_mag), window (N), basis -> (B*F, row_stride) windowed kernel rows.  Every
    call that takes a window ends here, so this is where its length is checked: the kernel reads N taps of it."""
    B, F, n_mag = log_mag.shape
    if window.numel() != 2 * (n_mag - 1):
        raise _lib.GolfError(f"{design.kind}_fir: window has {window.numel()} taps, expected {2 * (n_mag - 1)}")
    lib = _lib.load()
    KS = lib.golf_zero_phase_fir_row_stride(n_mag)
    kern = torch.empty(B * F, KS, dtype=torch.float32, device=log_mag.device)
    _lib.check(getattr(lib, design.kernels)(log_mag.data_ptr(), window.data_ptr(), basis.data_ptr(), kern.data_ptr(),
                                            B * F, n_mag, _lib.stream_ptr()),
               design.kernels)
    return kern


def _fir_kernels(design: _FIRDesign, log_mag: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    _lib.require_device(log_mag, window)
    log_mag = log_mag.detach().contiguous()
    B, F, n_mag = log_mag.shape
    kern = _fir_kernels_raw(design, log_mag, window.contiguous(), _fir_basis(design, n_mag, log_mag.device))
    return kern.view(B, F, -1)[..., :2 * (n_mag - 1)]


def zero_phase_fir_kernels(log_mag: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """(B,F,n_mag) log magnitudes -> (B,F,N) windowed zero-phase FIR kernels, N = 2*(n_mag-1) (no autograd)."""
    return _fir_kernels(ZERO_PHASE_FIR, log_mag, window)


def min_phase_fir_kernels(log_mag: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """(B,F,n_mag) log magnitudes -> (B,F,N) minimum-phase FIR kernels times ``window`` (N taps), N = 2*(n_mag-1)
    (no autograd)."""
    return _fir_kernels(MIN_PHASE_FIR, log_mag, window)


class _FIRKernels(torch.autograd.Function):
    """(B,F,n_mag) log magnitudes -> (B*F, row_stride) windowed FIR rows of ``design``, on the MFMAs (zero-phase: a cosine
    transform; minimum-phase: two contractions)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, log_mag, window, design):
        _lib.require_device(log_mag, window)
        log_mag = log_mag.contiguous()
        window = window.contiguous()
        basis = _fir_basis(design, log_mag.shape[2], log_mag.device)
        kern = _fir_kernels_raw(design, log_mag, window, basis)
        ctx.save_for_backward(log_mag, window, basis)
        ctx.design = design
        return kern

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_kern):
        log_mag, window, basis = ctx.saved_tensors
        name = ctx.design.kernels_bwd
        g_kern = g_kern.contiguous()
        B, F, n_mag = log_mag.shape
        g_lm = torch.empty_like(log_mag)
        _lib.check(getattr(_lib.load(), name)(g_kern.data_ptr(), log_mag.data_ptr(), window.data_ptr(), basis.data_ptr(),
                                              g_lm.data_ptr(), B * F, n_mag, _lib.stream_ptr()),
                   name)
        return g_lm, None, None


def _fir_frames_name(causal: bool) -> str:
    return "fir_frames_causal" if causal else "fir_frames"


def _fir_frames_length(causal: bool, T: int, F: int, N: int, hop: int) -> int:
    lib = _lib.load()
    n = getattr(lib, f"golf_ltv_{_fir_frames_name(causal)}_length")(T, F, N, hop)
    if n < 0:
        raise _lib.GolfError(lib.golf_last_error().decode(errors="replace"))
    return n


def fir_frames_length(T: int, F: int, N: int, hop: int) -> int:
    return _fir_frames_length(False, T, F, N, hop)


def fir_frames_causal_length(T: int, F: int, N: int, hop: int) -> int:
    return _fir_frames_length(True, T, F, N, hop)


class _FIRFrames(torch.autograd.Function):
    """Per-frame FIR with kernel rows kern (B*F, row_stride); output frame f uses row f + frame0.  Zero-phase alignment:
    y[b,f*hop+n] = sum_k kern[f+frame0][k] pad(ex)[b,f*hop+n+k]; ``causal``: sum_j kern[f+frame0][j] ex[b,f*hop+n-j]."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, kern, F, N, hop, frame0, causal):
        _lib.require_device(ex, kern)
        lib = _lib.load()
        who = _fir_frames_name(causal)
        ex = _rows(ex)
        kern = kern.contiguous()
        B, T = ex.shape
        if kern.shape[0] != B * F:
            raise _lib.GolfError(f"{who}: {kern.shape[0]} kernel rows for B={B}, F={F}")
        Ty = _fir_frames_length(causal, T, F - frame0, N, hop)
        y = torch.empty(B, Ty, dtype=torch.float32, device=ex.device)
        name = f"golf_ltv_{who}_fwd_f32"
        _lib.check(getattr(lib, name)(ex.data_ptr(), ex.stride(0), kern.data_ptr(), kern.shape[1], y.data_ptr(),
                                      y.stride(0), B, T, F, N, hop, frame0, _lib.stream_ptr()),
                   name)
        ctx.save_for_backward(ex, kern)
        ctx.geom = (F, N, hop, frame0, causal)
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        ex, kern = ctx.saved_tensors
        F, N, hop, frame0, causal = ctx.geom
        gy = _rows(gy)
        B, T = ex.shape
        need_ex, need_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_ex = torch.empty_like(ex) if need_ex else None
        g_kern = torch.empty_like(kern) if need_k else None
        name = f"golf_ltv_{_fir_frames_name(causal)}_bwd_f32"
        _lib.check(getattr(_lib.load(), name)(gy.data_ptr(), gy.stride(0), ex.data_ptr(), ex.stride(0),
                                              kern.data_ptr(), kern.shape[1],
                                              g_ex.data_ptr() if need_ex else None,
                                              g_ex.stride(0) if need_ex else 0,
                                              g_kern.data_ptr() if need_k else None,
                                              B, T, F, N, hop, frame0, _lib.stream_ptr()),
                   name)
        # (the padding taps [N, row stride) carry no gradient: the kernel writes their zeros itself)
        return g_ex, g_kern, None, None, None, None, None


def _check_causal_frames(who: str, ex, F: int, hop: int) -> None:
    T = ex.shape[-1]
    if T < hop:
        raise _lib.GolfError(f"{who}: excitation (T={T}) shorter than one hop ({hop})")
    if T // hop > F:   # the reference asserts this (models/filters.py:273-275)
        raise _lib.GolfError(f"{who}: {T // hop} frames of excitation (T={T}, hop={hop}) but only {F} kernels")


def _check_fir_inputs(who: str, ex, log_mag) -> None:
    if log_mag.dim() != 3 or ex.dim() != 2 or log_mag.shape[0] != ex.shape[0]:
        raise _lib.GolfError(f"{who}: ex {tuple(ex.shape)} vs log_mag {tuple(log_mag.shape)}")


def _fir_filter(design: _FIRDesign, ex, log_mag, window, hop: int) -> torch.Tensor:
    who = f"{design.kind}_fir_filter"
    _check_fir_inputs(who, ex, log_mag)
    F, n_mag = log_mag.shape[1], log_mag.shape[2]
    if design.causal:
        _check_causal_frames(who, ex, F, hop)
    kern = _FIRKernels.apply(log_mag, window, design)
    return _FIRFrames.apply(ex, kern, F, 2 * (n_mag - 1), hop, 0, design.causal)


def zero_phase_fir_filter(ex: torch.Tensor, log_mag: torch.Tensor, window: torch.Tensor, hop: int) -> torch.Tensor:
    """LTVZeroPhaseFIRFilter.forward on plain tensors: ex (B,T), log_mag (B,F,n_mag) at ``hop`` -> (B, nfr*hop);
    differentiable w.r.t. ex and log_mag."""
    return _fir_filter(ZERO_PHASE_FIR, ex, log_mag, window, hop)


def min_phase_fir_filter(ex: torch.Tensor, log_mag: torch.Tensor, window: torch.Tensor, hop: int) -> torch.Tensor:
    """LTVMinimumPhaseFIRFilter.forward on plain tensors: ex (B,T), log_mag (B,F,n_mag) at ``hop``, window (N) ->
    (B, (T // hop) * hop), y[b,f*hop+n] = sum_j kernel[b,f,j] ex[b,f*hop+n-j]; differentiable w.r.t. ex and log_mag."""
    return _fir_filter(MIN_PHASE_FIR, ex, log_mag, window, hop)


def _fir_filter_precise(design: _FIRDesign, ex, log_mag, window, hop: int) -> torch.Tensor:
    """The kernels linearly interpolated to sample rate, as two frame FIRs (kernel rows f and f+1 over the same signal)
    blended per sample; the single sample t = (F-1)*hop is a dot product with the last kernel.  The designs differ in
    the lead L, the samples of left context an output reads: y[t] = sum_k K_t[k] ex[t + k - L] (zero-phase) or
    sum_j K_t[j] ex[t - j] (causal, L = N-1, the window of ex reversed)."""
    who = f"{design.kind}_fir_filter_precise"
    _check_fir_inputs(who, ex, log_mag)
    B, T = ex.shape
    F, n_mag = log_mag.shape[1], log_mag.shape[2]
    if F < 2:
        raise _lib.GolfError(f"{who}: need at least 2 frames")
    N = 2 * (n_mag - 1)
    L = N - 1 if design.causal else (N - 1) // 2
    Tfull = (F - 1) * hop + 1
    Tout = min(T, Tfull)
    kern = _FIRKernels.apply(log_mag, window, design)
    # the samples the outputs t < Tfull can reach: indices < Tfull + N-1-L (zeros past T); causal: nothing later than t
    Tin = Tfull + N - 1 - L
    x = ex[:, :Tin]
    if x.shape[1] < Tin:
        x = torch.nn.functional.pad(x, (0, Tin - x.shape[1]))
    ya = _FIRFrames.apply(x, kern, F, N, hop, 0, design.causal)[:, : (F - 1) * hop]
    yb = _FIRFrames.apply(x, kern, F, N, hop, 1, design.causal)[:, : (F - 1) * hop]
    w = (torch.arange((F - 1) * hop, device=ex.device) % hop).to(torch.float32) / hop
    main = ya + w * (yb - ya)
    tail = torch.nn.functional.pad(x, (L, 0))[:, Tfull - 1: Tfull - 1 + N]  # ex[Tfull-1 - L + i], i < N
    if design.causal:
        tail = tail.flip(-1)   # the signal, not the kernel: the order of the products in the sum stays the kernel's
    last = (tail * kern.view(B, F, -1)[:, F - 1, :N]).sum(-1, keepdim=True)
    return torch.cat([main, last], dim=1)[:, :Tout]


def zero_phase_fir_filter_precise(ex: torch.Tensor, log_mag: torch.Tensor, window: torch.Tensor, hop: int) -> torch.Tensor:
    """LTVZeroPhaseFIRFilterPrecise.forward (reference models/filters.py:308-337): the kernels are linearly
    interpolated to sample rate, y[t] = sum_k pad(ex)[t+k] * ((1-w_t) K_f[k] + w_t K_{f+1}[k]), f = t // hop,
    w_t = (t % hop)/hop, output length min(T, (F-1)*hop+1).  Evaluated as two frame FIRs (kernel rows f and f+1 over
    the same signal) blended per sample; the single sample t = (F-1)*hop is a dot product with the last kernel."""
    return _fir_filter_precise(ZERO_PHASE_FIR, ex, log_mag, window, hop)


def min_phase_fir_filter_precise(ex: torch.Tensor, log_mag: torch.Tensor, window: torch.Tensor, hop: int) -> torch.Tensor:
    """LTVMinimumPhaseFIRFilterPrecise.forward (reference models/filters.py:223-241): the kernels are linearly
    interpolated to sample rate, y[t] = sum_j ((1-w_t) K_f[j] + w_t K_{f+1}[j]) ex[t-j], f = t // hop, w_t = (t % hop)/hop,
    output length min(T, (F-1)*hop+1).  Evaluated as two causal frame FIRs (kernel rows f and f+1 over the same signal)
    blended per sample; the single sample t = (F-1)*hop is a dot product with the last kernel."""
    return _fir_filter_precise(MIN_PHASE_FIR, ex, log_mag, window, hop)


def _ltv_fir_frames(causal: bool, ex, kernels, hop: int) -> torch.Tensor:
    B, F, N = kernels.shape
    if causal:
        _check_causal_frames("ltv_fir_frames_causal", ex, F, hop)
    KS = (N + 15) // 16 * 16
    kern = torch.nn.functional.pad(kernels.reshape(B * F, N), (0, KS - N))
    return _FIRFrames.apply(ex, kern, F, N, hop, 0, causal)


def ltv_fir_frames(ex: torch.Tensor, kernels: torch.Tensor, hop: int) -> torch.Tensor:
    """Frame-wise FIR with arbitrary per-frame kernels (B,F,N): y[b,f*hop+n] = sum_k pad(ex)[b,f*hop+n+k] *
    kernels[b,f,k]; differentiable w.r.t. both."""
    return _ltv_fir_frames(False, ex, kernels, hop)


def ltv_fir_frames_causal(ex: torch.Tensor, kernels: torch.Tensor, hop: int) -> torch.Tensor:
    """Causal frame-wise FIR with arbitrary per-frame kernels (B,F,N): y[b,f*hop+n] = sum_j kernels[b,f,j] *
    ex[b,f*hop+n-j], (T // hop) * hop samples; differentiable w.r.t. both."""
    return _ltv_fir_frames(True, ex, kernels, hop)


# ------------------------------------------------------------------------------------------------
# LTI FIR shared by the batch (room filter, reference models/filters.py:426-449)
# ------------------------------------------------------------------------------------------------
class _LTIFIR(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, taps, lead):
        _lib.require_device(ex, taps)
        lib = _lib.load()
        ex = _rows(ex)
        taps = taps.contiguous()
        B, T = ex.shape
        y = torch.empty(B, T, dtype=torch.float32, device=ex.device)
        _lib.check(lib.golf_lti_fir_f32(ex.data_ptr(), ex.stride(0), taps.data_ptr(), taps.numel(), lead,
                                        y.data_ptr(), y.stride(0), B, T, _lib.stream_ptr()), "golf_lti_fir_f32")
        ctx.save_for_backward(ex, taps)
        ctx.lead = lead
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        ex, taps = ctx.saved_tensors
        lib = _lib.load()
        gy = _rows(gy)
        B, T = ex.shape
        n = taps.numel()
        g_ex = g_taps = None
        if ctx.needs_input_grad[0]:
            g_ex = torch.empty_like(ex)
            # the adjoint = the same FIR with the taps in reverse order: a negative tap count (ABI 5) instead of taps.flip(0)
            _lib.check(lib.golf_lti_fir_f32(gy.data_ptr(), gy.stride(0), taps.data_ptr(), -n, n - 1 - ctx.lead,
                                            g_ex.data_ptr(), g_ex.stride(0), B, T, _lib.stream_ptr()),
                       "golf_lti_fir_f32 (adjoint)")
        if ctx.needs_input_grad[1]:
            g_taps = torch.empty_like(taps)
            ws = _workspace(lib.golf_lti_fir_taps_grad_workspace_bytes(B, T, n), ex.device)
            _lib.check(lib.golf_lti_fir_taps_grad_f32(gy.data_ptr(), gy.stride(0), ex.data_ptr(), ex.stride(0),
                                                      g_taps.data_ptr(), n, ctx.lead, B, T, ws.data_ptr(),
                                                      ws.numel(), _lib.stream_ptr()),
                       "golf_lti_fir_taps_grad_f32")
        return g_ex, g_taps, None


def lti_fir(ex: torch.Tensor, taps: torch.Tensor, lead: int) -> torch.Tensor:
    """y[b,t] = sum_n taps[n] * ex[b, t-lead+n] (zero outside the signal); taps.numel() % 4 == 0; differentiable
    w.r.t. both arguments."""
    return _LTIFIR.apply(ex, taps, lead)


# ------------------------------------------------------------------------------------------------
# harmonic oscillator bank (reference models/synth.py:403-547)
# ------------------------------------------------------------------------------------------------
def _up_len(n: int, hop: int) -> int:
    return (n - 1) * hop + 1 if hop > 1 else n


class _HarmonicOsc(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, phase, amp, tscale, hscale, H, phase_hop, amp_hop, ts_hop, phase_offset=None, po_hop=1,
                initial_phase=None):
        _lib.require_device(phase, amp, tscale, hscale, phase_offset, initial_phase)
        lib = _lib.load()
        phase = _rows(phase)
        B, Tp = phase.shape
        Tout = _up_len(Tp, phase_hop)
        Fa = Fs = 1
        if amp is not None:
            amp = amp.contiguous()
            if amp.dim() != 3 or amp.shape[0] != B or amp.shape[2] != H:
                raise _lib.GolfError(f"harmonic_osc: amplitudes {tuple(amp.shape)} for B={B}, H={H}")
            Fa = amp.shape[1]
            Tout = min(Tout, _up_len(Fa, amp_hop))
        if tscale is not None:
            tscale = tscale.contiguous()
            Fs = tscale.shape[1]
            Tout = min(Tout, _up_len(Fs, ts_hop))
        if hscale is not None:
            hscale = hscale.contiguous()
        Fo = 1
        if phase_offset is not None:
            phase_offset = phase_offset.contiguous()
            Fo = phase_offset.shape[1]
            Tout = min(Tout, _up_len(Fo, po_hop))
        if initial_phase is not None:
            initial_phase = initial_phase.contiguous()
            if tuple(initial_phase.shape) != (B, H):
                raise _lib.GolfError(f"harmonic_osc: initial_phase {tuple(initial_phase.shape)} for B={B}, H={H}")
        out = torch.empty(B, Tout, dtype=torch.float32, device=phase.device)
        ws = _workspace(lib.golf_harmonic_osc_workspace_bytes(B, Tp, phase_hop, Fa if amp is not None else 0, H),
                        phase.device)
        rc = lib.golf_harmonic_osc_fwd_f32(phase.data_ptr(), phase.stride(0), Tp, phase_hop, _lib.ptr(amp), Fa, amp_hop,
                                           _lib.ptr(tscale), Fs, ts_hop, _lib.ptr(hscale), H, out.data_ptr(),
                                           out.stride(0), B, Tout, ws.data_ptr(), ws.numel(), _lib.stream_ptr(),
                                           _lib.ptr(phase_offset), Fo, po_hop, _lib.ptr(initial_phase))
        _lib.check(rc, "golf_harmonic_osc_fwd_f32")
        ctx.save_for_backward(phase, tscale, hscale, amp, phase_offset, initial_phase)
        ctx.geom = (H, phase_hop, amp_hop, ts_hop, Fa, Fs, Tout, amp is not None)
        ctx.po = (Fo, po_hop)
        return out

    @staticmethod
    def _run(lib, name, phase, amp, tscale, hscale, geom, phase_offset=None, po=(1, 1), initial_phase=None):
        H, phase_hop, amp_hop, ts_hop, Fa, Fs, Tout, has_amp = geom
        B, Tp = phase.shape
        out = torch.empty(B, Tout, dtype=torch.float32, device=phase.device)
        ws = _workspace(lib.golf_harmonic_osc_workspace_bytes(B, Tp, phase_hop, Fa if has_amp else 0, H), phase.device)
        rc = getattr(lib, name)(phase.data_ptr(), phase.stride(0), Tp, phase_hop, _lib.ptr(amp), Fa, amp_hop,
                                _lib.ptr(tscale), Fs, ts_hop, _lib.ptr(hscale), H, out.data_ptr(), out.stride(0), B, Tout,
                                ws.data_ptr(), ws.numel(), _lib.stream_ptr(), _lib.ptr(phase_offset), po[0], po[1],
                                _lib.ptr(initial_phase))
        _lib.check(rc, name)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_out):
        phase, tscale, hscale, amp, phase_offset, initial_phase = ctx.saved_tensors
        H, phase_hop, amp_hop, ts_hop, Fa, Fs, Tout, has_amp = ctx.geom
        if ctx.needs_input_grad[3]:
            raise NotImplementedError("golf_amd: the per-harmonic scale of the harmonic oscillator is a constant "
                                      "(SawToothOscillator's 1/h buffer)")
        lib = _lib.load()
        g_out = _rows(g_out.float())
        B, Tp = phase.shape
        g_phase = g_amp = g_ts = g_po = g_ip = None
        if ctx.needs_input_grad[10]:
            # d out / d initial_phase[b,h] = 2 pi sum_t g[t] A_h[t] cos(2 pi theta_h[t]), A = the (masked, scaled) amplitude
            # track.  cos(x) = sin(x + 1/4 cycle) and A_h[t] = sum_f hat_f(t) amp[b,f,h]: the amplitude-gradient kernel run
            # with initial_phase + 1/4 returns G[b,f,h] = sum_t hat_f(t) g[t] cos(.) (scales and Nyquist mask included), and
            # g_ip = 2 pi sum_f amp[b,f,h] G[b,f,h].  Without an amplitude track (A = 1): pseudo-frames 256 samples apart, whose
            # hat functions sum to one over the signal -- G summed over them is the plain sum over t.  (Two frames one whole
            # signal apart gave the kernel ONE segment: a single wave per utterance walking Tout x H sincos chains, milliseconds
            # per call -- ADVICE r3.)  (reference: autograd through models/synth.py:434-440)
            if has_amp:
                Fq, hq = Fa, amp_hop
            else:
                hq = 256 if Tout > 257 else max(Tout - 1, 1)
                Fq = -(-(Tout - 1) // hq) + 1 if Tout > 1 else 2
            G = torch.empty(B, Fq, H, dtype=torch.float32, device=phase.device)
            ws = _workspace(lib.golf_harmonic_osc_workspace_bytes(B, Tp, phase_hop, Fq, H), phase.device)
            shifted = (initial_phase + 0.25).contiguous()
            rc = lib.golf_harmonic_osc_bwd_amp_f32(g_out.data_ptr(), g_out.stride(0), phase.data_ptr(),
                                                   phase.stride(0), Tp, phase_hop, Fq, hq, _lib.ptr(tscale), Fs,
                                                   ts_hop, _lib.ptr(hscale), H, G.data_ptr(), B, Tout,
                                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr(), _lib.ptr(phase_offset),
                                                   ctx.po[0], ctx.po[1], shifted.data_ptr())
            _lib.check(rc, "golf_harmonic_osc_bwd_amp_f32")
            g_ip = (2.0 * math.pi) * ((G * amp).sum(1) if has_amp else G.sum(1))
        if has_amp and ctx.needs_input_grad[1]:
            g_amp = torch.empty(B, Fa, H, dtype=torch.float32, device=phase.device)
            ws = _workspace(lib.golf_harmonic_osc_workspace_bytes(B, Tp, phase_hop, Fa, H), phase.device)
            rc = lib.golf_harmonic_osc_bwd_amp_f32(g_out.data_ptr(), g_out.stride(0), phase.data_ptr(),
                                                   phase.stride(0), Tp, phase_hop, Fa, amp_hop, _lib.ptr(tscale), Fs,
                                                   ts_hop, _lib.ptr(hscale), H, g_amp.data_ptr(), B, Tout,
                                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr(), _lib.ptr(phase_offset),
                                                   ctx.po[0], ctx.po[1], _lib.ptr(initial_phase))
            _lib.check(rc, "golf_harmonic_osc_bwd_amp_f32")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[8]:
            # out depends on the phase input through Phi = cumsum(up(phase)) (the Nyquist mask is piecewise constant):
            # g_phase = up^T( reverse-cumsum( g_out * d out / d Phi ) ), the derivative bank from the same kernel
            d = _HarmonicOsc._run(lib, "golf_harmonic_osc_dphase_f32", phase, amp if has_amp else None, tscale, hscale,
                                  ctx.geom, phase_offset, ctx.po, initial_phase)
            g_inst = (g_out[:, :Tout] * d).double()
            if ctx.needs_input_grad[0]:
                g_up = torch.flip(torch.cumsum(torch.flip(g_inst, [1]), 1), [1]).float()
                g_phase = upsample_adjoint(g_up, phase_hop, Tp)
            if ctx.needs_input_grad[8]:   # the offset enters every harmonic's phase like Phi does, without the cumsum
                g_po = upsample_adjoint(g_inst.float(), ctx.po[1], ctx.po[0])
        if tscale is not None and ctx.needs_input_grad[2]:
            # out = up(tscale) * S: S is the same kernel without the per-sample scale
            # ... and its length is the output's only while another track is as short as tscale: a tscale that alone ends
            # the output rides along as ones (acc * 1.0f: the same bits)
            others = [_up_len(Tp, phase_hop)] + ([_up_len(Fa, amp_hop)] if has_amp else []) \
                + ([_up_len(*ctx.po)] if phase_offset is not None else [])
            unit = None if min(others) == Tout else torch.ones_like(tscale)
            geom = (H, phase_hop, amp_hop, ts_hop, Fa, 1 if unit is None else Fs, Tout, has_amp)
            S = _HarmonicOsc._run(lib, "golf_harmonic_osc_fwd_f32", phase, amp if has_amp else None, unit, hscale, geom,
                                  phase_offset, ctx.po, initial_phase)
            g_ts = upsample_adjoint(g_out[:, :Tout] * S, ts_hop, Fs)
        return g_phase, g_amp, g_ts, None, None, None, None, None, g_po, None, g_ip


def upsample_adjoint(v: torch.Tensor, hop: int, F: int) -> torch.Tensor:
    """Adjoint of linear_upsample along dim 1: v (B,T) with T <= (F-1)*hop+1 -> (B,F)."""
    B, T = v.shape
    out = v.new_zeros(B, F)
    if hop == 1 or F == 1:
        out[:, :T] = v
        return out
    # sample f*hop + r gives (1 - r/hop) of itself to frame f and r/hop to frame f+1; the last one, (F-1)*hop, is frame F-1's
    # alone.  Plain reductions over r: index_add_ sums with atomics, in an order (and to a last bit) that varies between calls
    L = (F - 1) * hop
    vp = torch.nn.functional.pad(v, (0, L + 1 - T))
    seg = vp[:, :L].reshape(B, F - 1, hop)
    w = torch.arange(hop, device=v.device, dtype=v.dtype) / hop
    out[:, :F - 1] = (seg * (1 - w)).sum(-1)
    out[:, 1:] += (seg * w).sum(-1)
    out[:, F - 1] += vp[:, L]
    return out


def harmonic_osc(phase, H: int, phase_hop: int = 1, amp=None, amp_hop: int = 1, tscale=None, ts_hop: int = 1,
                 hscale=None, phase_offset=None, po_hop: int = 1, initial_phase=None) -> torch.Tensor:
    """out[t] = sum_h [h p(t) < 0.5] * up(amp)[t,h] * up(tscale)[t] * hscale[h]
                      * sin(2 pi (h (cumsum(p)[t] + up(phase_offset)[t]) + initial_phase[b,h])),   p = up(phase);
    differentiable w.r.t. ``amp``, ``phase``, ``tscale``, ``phase_offset`` and ``initial_phase`` (reference models/synth.py:403-446)."""
    return _HarmonicOsc.apply(phase, amp, tscale, hscale, H, phase_hop, amp_hop, ts_hop, phase_offset, int(po_hop),
                              initial_phase)


def harmonic_osc_stream(phase, j0: int, nseg: int, final_point: bool, phase_hop: int, H: int, acc: torch.Tensor, amp=None,
                        a_first: int = 0, a_end: int = -1, amp_hop: int = 1, tscale=None, s_first: int = 0, s_end: int = -1,
                        ts_hop: int = 1, hscale=None) -> torch.Tensor:
    """``harmonic_osc``'s output samples of coarse phase segments j0 .. j0+nseg-1 (+ the utterance's last sample with
    ``final_point``) from the carried Q0.64 phase ``acc`` ((B,) int64 holding the uint64 bits, updated in place):
    golf_harmonic_osc_stream_f32, bit for bit the one-shot's samples at the same global indices.  ``phase`` (B, >= nseg+1)
    holds p[j0 ..]; ``amp`` (B, na, H) rows a_first .. and ``tscale`` (B, ns) rows s_first .. of their tracks, ``a_end`` /
    ``s_end`` the tracks' row counts once they have ended (-1 before).  Returns (B, nseg*P + final_point).  Inference only;
    fp16 / bf16 tracks are cast to fp32 first."""
    _inference_only("harmonic_osc_stream", phase, amp, tscale, hscale)
    phase = _rows(phase.float())
    amp = None if amp is None else amp.float().contiguous()
    tscale = None if tscale is None else _rows(tscale.float())
    hscale = None if hscale is None else hscale.float().contiguous()
    _lib.require_device(phase, amp, tscale, hscale)
    B = phase.shape[0]
    if not acc.is_cuda or acc.dtype != torch.int64 or acc.shape != (B,):
        raise _lib.GolfError(f"harmonic_osc_stream: acc must be a ({B},) int64 device tensor")
    if phase.shape[1] < int(nseg) + 1:
        raise _lib.GolfError(f"harmonic_osc_stream: {phase.shape[1]} phase samples for {nseg} segments")
    if amp is not None and (amp.dim() != 3 or amp.shape[0] != B or amp.shape[2] != H):
        raise _lib.GolfError(f"harmonic_osc_stream: amplitudes {tuple(amp.shape)} for B={B}, H={H}")
    if tscale is not None and tscale.shape[0] != B:
        raise _lib.GolfError(f"harmonic_osc_stream: tscale {tuple(tscale.shape)} for B={B}")
    if hscale is not None and hscale.numel() != H:
        raise _lib.GolfError(f"harmonic_osc_stream: hscale of {hscale.numel()} values for H={H}")
    nall = int(nseg) + int(bool(final_point))
    out = torch.empty(B, int(nseg) * int(phase_hop) + int(bool(final_point)), dtype=torch.float32, device=phase.device)
    ws = _workspace(8 * B * nall, phase.device) if nall else None
    lib = _lib.load()
    rc = lib.golf_harmonic_osc_stream_f32(phase.data_ptr(), phase.stride(0), int(nseg), int(bool(final_point)), int(phase_hop),
                                          _lib.ptr(amp), int(a_first), 0 if amp is None else amp.shape[1], int(a_end),
                                          int(amp_hop), _lib.ptr(tscale), 0 if tscale is None else tscale.stride(0),
                                          int(s_first), 0 if tscale is None else tscale.shape[1], int(s_end), int(ts_hop),
                                          _lib.ptr(hscale), int(H), int(j0), acc.data_ptr(), out.data_ptr(),
                                          max(1, out.stride(0)), B, _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                          _lib.stream_ptr())
    _lib.check(rc, "golf_harmonic_osc_stream_f32")
    return out


# ------------------------------------------------------------------------------------------------
# frame-wise all-pole synthesis as a cascade of biquads (reference models/lpc.py:94-131)
# ------------------------------------------------------------------------------------------------
class _BiquadFramesOLA(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, ex, gain, biquads, window, hop, pad, frame_gain):
        _lib.require_device(ex, gain, biquads, window)
        lib = _lib.load()
        ex = _rows(ex)
        gain, biquads, window = gain.contiguous(), biquads.contiguous(), window.contiguous()
        B, Tx0 = ex.shape
        F, K = biquads.shape[1], biquads.shape[2]
        W = window.numel()
        Tx = Tx0 if frame_gain else min(Tx0, (F - 1) * hop + 1)
        nfr = (Tx + 2 * pad - W) // hop + 1
        if nfr < 1 or nfr > F:
            raise _lib.GolfError(f"biquad_frames_ola: {nfr} frames for {F} coefficient frames")
        Ty = (nfr - 1) * hop + W - 2 * pad
        y = torch.empty(B, Ty, dtype=torch.float32, device=ex.device)
        ws = _workspace(B * nfr * W * 4 + 256, ex.device)
        rc = lib.golf_biquad_frames_ola_fwd_f32(ex.data_ptr(), ex.stride(0), gain.data_ptr(), biquads.data_ptr(),
                                                window.data_ptr(), y.data_ptr(), y.stride(0), B, Tx, F, K, hop, W, pad,
                                                1 if frame_gain else 0, Ty, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "golf_biquad_frames_ola_fwd_f32")
        ctx.geom = (hop, pad, bool(frame_gain), Tx, nfr, Ty)
        ctx.save_for_backward(ex, gain, biquads, window)
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        ex, gain, biquads, window = ctx.saved_tensors
        hop, pad, frame_gain, Tx, nfr, Ty = ctx.geom
        lib = _lib.load()
        B, Tx0 = ex.shape
        F, K = biquads.shape[1], biquads.shape[2]
        W = window.numel()
        # the overlap-add of the window (the normaliser of the forward), on the output samples: nfr copies of the window
        # folded hop apart.  (Not conv_transpose1d: for one (1,1,nfr) x (1,1,W) call the convolution library times every
        # solver it has on the device first, and at nfr = 15, W = 100, hop = 24 one of them left the device with a
        # memory-access fault; fold is a plain gather, the same bits on every call.)
        norm = torch.nn.functional.fold(window.view(1, W, 1).expand(1, W, nfr), (1, (nfr - 1) * hop + W), (1, W),
                                        stride=(1, hop))
        norm = norm.view(-1)[pad: pad + Ty]
        gq = _rows((gy.float() / norm).contiguous())
        g_ex = torch.zeros(B, Tx0, dtype=torch.float32, device=ex.device)
        g_bq = torch.empty_like(biquads)
        g_gain_f = torch.empty_like(gain)
        gxe = torch.empty(B, Tx, dtype=torch.float32, device=ex.device)
        ws = _workspace(lib.golf_biquad_frames_bwd_workspace_bytes(B, Tx, F, K, hop, W, pad), ex.device)
        rc = lib.golf_biquad_frames_ola_bwd_f32(gq.data_ptr(), gq.stride(0), ex.data_ptr(), ex.stride(0), gain.data_ptr(),
                                                biquads.data_ptr(), window.data_ptr(), g_ex.data_ptr(), g_ex.stride(0),
                                                g_gain_f.data_ptr(), g_bq.data_ptr(), gxe.data_ptr(), B, Tx, F, K, hop, W,
                                                pad, 1 if frame_gain else 0, Ty, ws.data_ptr(), ws.numel(),
                                                _lib.stream_ptr())
        _lib.check(rc, "golf_biquad_frames_ola_bwd_f32")
        g_gain = g_gain_f if frame_gain else upsample_adjoint(gxe, hop, F)
        return g_ex, g_gain, g_bq, None, None, None, None


def biquad_frames_ola(ex: torch.Tensor, gain: torch.Tensor, biquads: torch.Tensor, window: torch.Tensor, hop: int,
                      pad: int = None, frame_gain: bool = True) -> torch.Tensor:
    """ex (B,Tx), gain (B,F), biquads (B,F,K,3) -> (B,Ty): every frame through its K sections 1/(a0+a1 z^-1+a2 z^-2),
    windowed overlap-add.  ``pad`` defaults to (W-hop)//2 and ``frame_gain`` to True (BatchSecondOrderLPCSynth);
    pad = W//2, frame_gain=False is LTVMinimumPhaseFilter's convention.  Differentiable w.r.t. ex, gain and biquads
    (custom HIP backward: the cascade's adjoint is the reversed cascade on the reversed signal)."""
    W = window.numel()
    pad = (W - hop) // 2 if pad is None else pad
    return _BiquadFramesOLA.apply(ex, gain, biquads, window, int(hop), int(pad), bool(frame_gain))
