"""Streaming GOLF synthesis: the decoder fed control frames as they are produced, audio returned block by block.

``DecoderStream(decoder, batch_size)`` wraps a ``SourceFilterSynth`` as golf-ss builds it.  Every ``push`` hands over the NEXT
slice of each input track (any length, 0 included) and returns the output samples that the inputs pushed so far determine;
``finish()`` returns the rest, with the utterance's edges treated exactly as the one-shot call treats them.  The concatenation of
all outputs is ``decoder(...)`` on the concatenated inputs (INTEGRATION.md "Streaming synthesis").

Per stage, what crosses a block boundary:
  oscillator     the exact Q0.64 phase accumulator (golf_glottal_osc_stream_f32) and the last (K-1)/2 fine samples of the
                 decimator's context (golf_decimate_fir_f32 over an overlap window)
  noise filter   the noise and kernel rows of the frames still to come (golf_ltv_fir_frames_fwd_f32 over a window that starts
                 ceil(P/hop) frames early, those frames dropped)
  end filter     the last M outputs (golf_ltv_allpole_fwd_state_f32, the serial recursion)
  room filter    the last ``lead`` end-filter outputs (golf_lti_fir_f32 over an overlap window)
All of it is device memory; ``push`` reads nothing back from the device.  The bookkeeping is host integers derived from the
pushed lengths alone: ``emit_count`` and ``final_lengths`` below are pure functions of them and of ``StreamGeometry``.

``FramewiseDecoderStream(decoder, batch_size)`` does the same for the two decoders built on the frame-wise LPC filter
(LTVMinimumPhaseFilter): golf-ff (SourceFilterSynth, the filter as its end filter) and golf-v1 (HarmonicPlusNoiseSynth, the
filter on the oscillator, the room filter as its end filter).  The filter's stage carries its last ceil(W/hop) - 1 filtered
frames (golf_lti_frames_ola_stream_f32): every frame is filtered once, as soon as its samples and controls are there.
``open_stream`` returns whichever of the two classes fits a decoder.

``HarmonicPlusNoiseStream(decoder, batch_size)`` streams the other harmonic-plus-noise decoders (DDSP, the ISMIR'23 ddsp /
sawsing / pulse / glottal_d vocoders, golf-v1 too): the harmonic oscillator bank from a carried Q0.64 phase
(golf_harmonic_osc_stream_f32) or the glottal table as above, and on each branch PassThrough, the zero-phase FIR or the
frame-wise LPC filter (centred or not), each branch with its own carry.  It is opened explicitly: ``open_stream`` keeps its
choice between the two classes above.  Its bookkeeping is ``hpn_emit_count`` / ``hpn_final_lengths`` / ``hpn_stream_latency``
over ``HPNGeometry``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

from . import _lib
from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["BranchGeometry", "DecoderStream", "FramewiseDecoderStream", "HPNGeometry", "HarmonicPlusNoiseStream",
           "StreamGeometry", "emit_count", "final_lengths", "hpn_emit_count", "hpn_final_lengths", "hpn_stream_latency",
           "open_stream", "stream_latency"]


@dataclass(frozen=True)
class StreamGeometry:
    """What the block bookkeeping depends on.  Hops are in output samples."""
    hop: int            # LPC hop of gain / a
    phase_hop: int      # hop of the phase track
    os: int             # oscillator oversampling
    half: int           # (K-1)/2 taps of the decimator (0 without oversampling)
    w_hop: int          # hop of the table-select track
    fir_taps: int = 0   # noise filter taps N = 2*(n_mag-1); 0: no noise filter
    fir_hop: int = 1    # hop of the noise filter's log magnitudes
    window: int = 0     # frame length W of the frame-wise LPC filter; 0: the sample-wise end filter (golf-ss)
    hpn: bool = False   # golf-v1 layout: the frame-wise filter on the oscillator alone, the filtered noise added after it

    @property
    def pad(self) -> int:
        return self.window // 2

    @property
    def P(self) -> int:
        return self.phase_hop * self.os

    @property
    def fir_lookahead(self) -> int:   # R = N-1-P of the zero-phase FIR: samples it reads after the one it writes
        return self.fir_taps - 1 - (self.fir_taps - 1) // 2 if self.fir_taps else 0


def _osc_len(g: StreamGeometry, n_phase: int) -> int:
    return GF.osc_lengths(n_phase, g.phase_hop, g.os)[1] if n_phase >= 1 else 0


def _osc_segments(g: StreamGeometry, n_phase: int, n_wsel: int) -> int:
    """Coarse phase segments j the oscillator can render before the inputs end: segment j reads p[j], p[j+1] and, for its fine
    samples m, table-select rows m // (w_hop*os) and the one after."""
    if n_phase < 2 or n_wsel < 2:
        return 0
    return max(0, min(n_phase - 1, ((n_wsel - 1) * g.w_hop * g.os) // g.P))


def _osc_outputs(g: StreamGeometry, fine: int) -> int:
    """Decimated outputs o whose taps (fine samples o*os - half .. o*os + half) all lie below ``fine``."""
    if g.os == 1:
        return fine
    return max(0, (fine - 1 - g.half) // g.os + 1)


def _noise_available(g: StreamGeometry, n_phase: int, n_noise: Optional[int]) -> int:
    """Noise samples certain to exist: the one-shot draws (or truncates the given noise to) the oscillator's length, which is
    at least the length the phase pushed so far implies."""
    lb = _osc_len(g, n_phase)
    return lb if n_noise is None else min(n_noise, lb)


def _fir_frames(g: StreamGeometry, n_noise_avail: int, n_logmag: int) -> int:
    """Noise-filter frames f whose reads (noise up to (f+1)*fir_hop - 1 + R) are all available."""
    return max(0, min(n_logmag, (n_noise_avail - g.fir_lookahead) // g.fir_hop))


def emit_count(g: StreamGeometry, n_phase: int, n_wsel: int, n_noise: Optional[int], n_logmag: int, n_gain: int,
               n_a: int) -> int:
    """E: the output samples [0, E) a stream emits once these many steps of each track have been pushed (``n_noise`` None: the
    noise is drawn on the device).  The largest multiple of ``hop`` such that every sample below it is determined -- through the
    operators' stencils -- by what has been pushed: osc (phase + table select, decimator context), filtered noise, and gain / a
    frames up to the one that closes the last sample's frame.
    Frame-wise filter (``g.window``): every sample whose frames (f <= (n + W/2) // hop) are all ready, see ``_ff_frames``."""
    if g.window:
        return _ff_emit(g, n_phase, n_wsel, n_noise, n_logmag, n_gain, n_a)[0]
    fine = _osc_segments(g, n_phase, n_wsel) * g.P
    n_src = _osc_outputs(g, fine)
    nz_avail = _noise_available(g, n_phase, n_noise)
    n_nz = _fir_frames(g, nz_avail, n_logmag) * g.fir_hop if g.fir_taps else nz_avail
    n_src = min(n_src, n_nz)
    return g.hop * max(0, min(n_src // g.hop, min(n_gain, n_a) - 1))


def final_lengths(g: StreamGeometry, n_phase: int, n_noise: Optional[int], n_logmag: int, n_frames: int) -> dict:
    """Lengths of the one-shot decoder's stages once the inputs have ended (``n_frames``: gain / a frames).  With the
    frame-wise filter also its input length (``filter_in``, the one-shot's Tx), frames (``frames``) and output length
    (``filter_out``); golf-v1's output is the shorter of the filtered oscillator and the filtered noise."""
    osc = _osc_len(g, n_phase)
    noise = osc if n_noise is None else min(n_noise, osc)
    if g.fir_taps:
        P = (g.fir_taps - 1) // 2
        span = noise + 2 * P - (g.fir_taps + g.fir_hop - 1)
        if span < 0:
            raise _lib.GolfError(f"DecoderStream: {noise} noise samples are shorter than one noise-filter frame span")
        nz = min(span // g.fir_hop + 1, n_logmag) * g.fir_hop
    else:
        nz = noise
    src = min(osc, nz)
    if g.window:
        x = osc if g.hpn else src
        Tx, nfr, Ty = GF.ff_output_length(x, n_frames, g.hop, g.window) if x >= 1 and n_frames >= 2 else (0, 0, 0)
        if nfr > n_frames:
            raise _lib.GolfError(f"frame-wise filter: {nfr} frames needed but only {n_frames} coefficient frames")
        return dict(osc=osc, noise=noise, noise_filter=nz, source=x, filter_in=Tx, frames=nfr, filter_out=Ty,
                    out=min(Ty, nz) if g.hpn else Ty)
    out = GF.ss_output_length(src, n_frames, g.hop) if n_frames >= 1 and src >= 1 else 0
    return dict(osc=osc, noise=noise, noise_filter=nz, source=src, out=out)


def stream_latency(g: StreamGeometry) -> int:
    """Worst-case lookahead in samples: output sample t is emitted at the latest once every track has been pushed up to input
    time t + latency (a track at hop h: its steps 0 .. (t + latency) // h).
        latency = hop - 1 + max(phase_hop + floor(half/os),             phase p[j+1] closes the decimator's last segment
                                w_hop + floor((half + P - 1)/os),       the table-select row after the one a sample sits in
                                fir_hop - 1 + R + phase_hop - 1,        the noise filter's frame (R = N-1-(N-1)//2 samples)
                                1)
    hop - 1 is the emission granularity (whole LPC frames).  golf-ss (hop 240, phase at hop 1, os 4, K 129, w_hop 2400,
    N 510): 239 + 2416 = 2655 samples.

    Frame-wise filter (``g.window`` = W, pad = W // 2, c = (W - pad - 1) // hop): sample t needs frame (t + pad) // hop, whose
    samples reach t + W - 1 and whose up(gain) reaches gain row (t + pad) // hop + c + 1, so
        latency = max(W - 1 + source lookahead,  pad + hop * (c + 1))
    where the source lookahead is the max(...) above (golf-v1: without the noise term, which then joins the outer max, since
    the filtered noise is added after the filter).  golf-ff (W 960, hop 240, the golf-ss source): 959 + 2416 = 3375."""
    if g.window:
        src = _src_lookahead(g, with_noise=not g.hpn)
        q = [g.window - 1 + src, g.pad + g.hop * ((g.window - g.pad - 1) // g.hop + 1)]
        if g.hpn:
            q.append(_noise_lookahead(g))
        return max(q)
    q = [g.phase_hop + g.half // g.os, g.w_hop + (g.half + g.P - 1) // g.os, 1]
    q.append(g.fir_hop - 1 + g.fir_lookahead + g.phase_hop - 1 if g.fir_taps else g.phase_hop - 1)
    return g.hop - 1 + max(q)


def _noise_lookahead(g: StreamGeometry) -> int:
    return g.fir_hop - 1 + g.fir_lookahead + g.phase_hop - 1 if g.fir_taps else g.phase_hop - 1


def _src_lookahead(g: StreamGeometry, with_noise: bool = True) -> int:
    """Input time past a source sample by which it is determined (the max(...) of ``stream_latency``)."""
    q = [g.phase_hop + g.half // g.os, g.w_hop + (g.half + g.P - 1) // g.os, 1]
    if with_noise:
        q.append(_noise_lookahead(g))
    return max(q)


def _ff_frames(g: StreamGeometry, n_x: int, n_gain: int, n_a: int) -> int:
    """Frames of the frame-wise filter that can be filtered while the utterance is open: frame f reads x up to
    f*hop - pad + W - 1 (all of it known: n_x samples), a[f], and gain rows up to seg + 1 for the segment seg of its last
    sample, (f*hop - pad + W - 1) // hop = f + c."""
    c = (g.window - g.pad - 1) // g.hop
    return max(0, min((n_x + g.pad - g.window) // g.hop + 1, n_a, n_gain - 1 - c))


def _ff_emit(g: StreamGeometry, n_phase: int, n_wsel: int, n_noise: Optional[int], n_logmag: int, n_gain: int,
             n_a: int) -> Tuple[int, int, int, int]:
    """(E, frames ready, filter samples finished, known filter input samples) while the utterance is open."""
    n_osc = _osc_outputs(g, _osc_segments(g, n_phase, n_wsel) * g.P)
    nz_avail = _noise_available(g, n_phase, n_noise)
    n_nz = _fir_frames(g, nz_avail, n_logmag) * g.fir_hop if g.fir_taps else nz_avail
    n_x = n_osc if g.hpn else min(n_osc, n_nz)
    nfr = _ff_frames(g, n_x, n_gain, n_a)
    n_y = max(0, nfr * g.hop - g.pad)     # samples whose last frame, (n + pad) // hop, is ready
    return (min(n_y, n_nz) if g.hpn else n_y), nfr, n_y, n_x


class _Track:
    """A device buffer of one input or intermediate track along dim 1, holding global steps [start, start + n)."""

    def __init__(self, start: int = 0, data: torch.Tensor = None):
        self.start = start
        self.data = data

    @property
    def end(self) -> int:
        return self.start + (0 if self.data is None else self.data.shape[1])

    def append(self, x: torch.Tensor) -> None:
        if x.shape[1] == 0 and self.data is not None:
            return
        self.data = x if self.data is None else torch.cat([self.data, x], 1)

    def get(self, lo: int, hi: int) -> torch.Tensor:
        assert self.start <= lo <= hi <= self.end, (self.start, lo, hi, self.end)
        return self.data[:, lo - self.start: hi - self.start]

    def drop_before(self, lo: int) -> None:
        lo = min(max(lo, self.start), self.end)
        if lo > self.start:
            self.data = self.data[:, lo - self.start:]
            self.start = lo


def _refuse(what: str):
    raise NotImplementedError(f"DecoderStream: {what} is not supported (streaming covers the golf-ss decoder: "
                              "SourceFilterSynth with an indexed glottal table, standard normal noise, the zero-phase FIR noise "
                              "filter or none, the sample-wise end filter, the LTI room filter or none)")


class _SourceStages:
    """The stages every GOLF stream shares: the carried-phase oscillator, the noise and its FIR filter, the room filter.
    Subclasses set ``B``, ``decoder``, ``generated_noise``, ``has_fir``, ``has_room`` and ``geometry`` (``_source_geometry``)
    before ``_setup_source``."""

    def _source_geometry(self, phase, wsel, a, lm, **frame_filter) -> StreamGeometry:
        osc = self.decoder.harm_oscillator
        os_ = int(osc.oversampling)
        taps = osc.decimater.taps.float().contiguous() if os_ > 1 else None
        self._taps = taps
        self._table = osc.table.detach().float().contiguous()
        return StreamGeometry(hop=int(a.hop_length), phase_hop=int(phase.hop_length), os=os_,
                              half=(taps.numel() - 1) // 2 if taps is not None else 0, w_hop=int(wsel.hop_length),
                              fir_taps=2 * (int(lm.shape[2]) - 1) if lm is not None else 0,
                              fir_hop=int(lm.hop_length) if lm is not None else 1, **frame_filter)

    def _setup_source(self, phase, lm, noise, room) -> None:
        dec = self.decoder
        g, B, dev = self.geometry, self.B, phase.device
        self._dev = dev
        # inputs (global steps), all on the device
        self._ph, self._w, self._g, self._a = _Track(), _Track(), _Track(), _Track()
        self._noise, self._kern = _Track(), _Track()
        self._noise_pushed = None if noise is None else 0
        self._lm_pushed = 0
        # oscillator: next segment to render, the exact phase before it, fine samples kept for the decimator
        self._seg = 0
        self._acc = torch.zeros(B, dtype=torch.int64, device=dev)
        pad = -(-g.half // g.os) * g.os   # zeros before fine sample 0: the one-shot decimator's own zero padding
        self._pre = _Track(-pad, torch.zeros(B, pad, device=dev))
        self._osc = _Track()
        self._nz = _Track()
        self._fir_frames = 0
        # room filter: taps and the zeros before sample 0
        if self.has_room:
            self._room_lead = room._padding
            self._room_taps = torch.cat([room.kernel.detach(), room._tail.to(room.kernel.dtype)]).float().contiguous()
            self._room_hist = torch.zeros(B, self._room_lead, device=dev)
        if lm is not None:
            self._fir_window = dec.noise_filter._window(g.fir_taps, dev)
            self._fir_basis = GF.zero_phase_fir_basis(int(lm.shape[2]), dev)

    def _check_hops(self, phase, wsel, gain, a, lm, noise):
        g = self.geometry
        want = [(phase, g.phase_hop, "phase"), (wsel, g.w_hop, "table select"), (gain, g.hop, "gain"), (a, g.hop, "a")]
        if lm is not None:
            want.append((lm, g.fir_hop, "log_mag"))
        if noise is not None:
            want.append((noise, 1, "noise"))
        for t, hop, name in want:
            if int(t.hop_length) != hop or t.shape[0] != self.B:
                raise ValueError(f"{type(self).__name__}.push: {name} of shape {tuple(t.shape)} at hop {t.hop_length}; "
                                 f"the stream has B={self.B}, hop {hop}")
        if a.shape[2] != self.M or (lm is not None and 2 * (lm.shape[2] - 1) != g.fir_taps):
            raise ValueError(f"{type(self).__name__}.push: the LPC order / noise-filter bins changed between pushes")
        if (noise is None) != (self._noise_pushed is None):
            raise ValueError(f"{type(self).__name__}.push: pass noise= in every push or in none")

    def _append(self, phase, wsel, gain, a, lm, noise):
        # (autocast: fp16 / bf16 control tracks become fp32 here, before any kernel sees them)
        f32 = lambda t: t.as_tensor().to(device=self._dev, dtype=torch.float32)
        self._ph.append(f32(phase))
        self._w.append(f32(wsel))
        self._g.append(f32(gain))
        self._a.append(f32(a).contiguous())
        if noise is not None:
            x = f32(noise)
            self._noise.append(x)
            self._noise_pushed += x.shape[1]
        if lm is not None and lm.shape[1]:
            x = f32(lm).contiguous()
            kern = GF._zp_kernels_raw(_lib.load(), x, self._fir_window, self._fir_basis)
            self._kern.append(kern.view(self.B, x.shape[1], -1))
        if lm is not None:
            self._lm_pushed += lm.shape[1]

    def _run_oscillator(self, n_osc: int, final: bool, g: StreamGeometry = None) -> None:
        g = self.geometry if g is None else g
        n_phase = self._ph.end
        nseg = (n_phase - 1 if n_phase >= 1 else 0) if final else _osc_segments(g, n_phase, self._w.end)
        last = final and n_phase >= 1
        if nseg > self._seg or last:
            j0 = self._seg
            ph = self._ph.get(j0, min(nseg + 1, n_phase))
            r_lo = min((j0 * g.P) // (g.w_hop * g.os), self._w.end - 1)   # (past the last row: the kernel repeats it)
            wsel = self._w.get(r_lo, self._w.end)
            pre = GF.glottal_osc_stream(ph, j0, nseg - j0, last, g.phase_hop, g.os, wsel, r_lo, g.w_hop, self._table,
                                        self.decoder.harm_oscillator.equal_energy, self._acc)
            self._pre.append(pre)
            self._seg = nseg
            self._ph.drop_before(nseg)   # p[nseg] closes the next segment
            self._w.drop_before(min((nseg * g.P) // (g.w_hop * g.os), self._w.end - 1))
        if n_osc <= self._osc.end:
            return
        if g.os == 1:
            self._osc.append(self._pre.get(self._osc.end, n_osc))
            self._pre.drop_before(n_osc)
            return
        x = self._pre.data
        o_base = self._pre.start // g.os
        out = GF.decimate_fir(x, self._taps, g.os)
        self._osc.append(out[:, self._osc.end - o_base: n_osc - o_base])
        keep = ((n_osc * g.os - g.half) // g.os) * g.os
        self._pre.drop_before(keep)

    def _run_noise(self, n_noise: int, n_nz: int, final: bool) -> None:
        g = self.geometry
        if self.generated_noise and n_noise > self._noise.end:
            self._noise.append(torch.randn(self.B, n_noise - self._noise.end, device=self._dev))
        if not self.has_fir:
            if n_nz > self._nz.end:
                self._nz.append(self._noise.get(self._nz.end, n_nz))
                self._noise.drop_before(n_nz)
            return
        f_lo, f_hi = self._fir_frames, n_nz // g.fir_hop
        if f_hi <= f_lo:
            return
        Pn = (g.fir_taps - 1) // 2
        q = -(-Pn // g.fir_hop)                       # frames whose left context would be the call's zero padding
        fs = max(0, f_lo - q)
        s0 = fs * g.fir_hop
        e = n_noise if final else min(n_noise, f_hi * g.fir_hop + g.fir_lookahead)
        x = self._noise.get(s0, e)
        kern = self._kern.data
        Fk = kern.shape[1]
        y = GF._FIRFrames.apply(x, kern.reshape(self.B * Fk, -1), Fk, g.fir_taps, g.fir_hop, fs - self._kern.start)
        self._nz.append(y[:, (f_lo - fs) * g.fir_hop: (f_hi - fs) * g.fir_hop])
        self._fir_frames = f_hi
        nxt = max(0, f_hi - q)
        self._noise.drop_before(nxt * g.fir_hop)
        self._kern.drop_before(nxt)

    def _run_room(self, y: torch.Tensor) -> torch.Tensor:
        if not self.has_room:
            return y
        lead = self._room_lead
        x = torch.cat([self._room_hist, y], 1)
        out = GF.lti_fir(x, self._room_taps, lead)[:, lead:]
        self._room_hist = x[:, x.shape[1] - lead:]
        return out


class DecoderStream(_SourceStages):
    """Block-by-block synthesis with a GOLF-ss ``SourceFilterSynth`` (see the module docstring and INTEGRATION.md).

    ``push(phase, harm_oscillator_params=(wsel,), noise_filter_params=(log_mag,), end_filter_params=(gain, a), noise=None)``
    takes AudioTensors holding the next slice of each track (hops as in the one-shot call) and returns a (B, n) fp32 tensor,
    n a multiple of the LPC hop; ``finish()`` returns the remainder.  ``noise=None`` draws N(0,1) on the device as
    StandardNormalNoise does; a decoder with another (value-independent) noise source needs ``noise`` in every push.
    ``latency`` (after the first push, which fixes the hops) is the worst-case lookahead in samples (``stream_latency``).
    Inference only; one stream for the whole batch (no per-row reset)."""

    def __init__(self, decoder, batch_size: int):
        from .ctrl import PassThrough
        from .filters import LTIAcousticFilter, LTVMinimumPhaseFilter, LTVMinimumPhaseFilterPrecise, LTVZeroPhaseFIRFilter
        from .noise import NoiseBand, SignFlipNoise, StandardNormalNoise, UniformNoise
        from .sf import SourceFilterSynth
        from .synth import IndexedGlottalFlowTable

        if not isinstance(decoder, SourceFilterSynth) or type(decoder).forward is not SourceFilterSynth.forward:
            _refuse(type(decoder).__name__)
        if decoder.subtract_harmonics:
            _refuse("subtract_harmonics=True")
        osc = decoder.harm_oscillator
        if not isinstance(osc, IndexedGlottalFlowTable) or type(osc).forward is not IndexedGlottalFlowTable.forward:
            _refuse(f"the oscillator {type(osc).__name__}")
        gen = decoder.noise_generator
        if isinstance(gen, (UniformNoise, SignFlipNoise, NoiseBand)) or getattr(gen, "uses_reference_values", True):
            _refuse(f"the noise generator {type(gen).__name__}")
        nf = decoder.noise_filter
        if not (type(nf) is PassThrough or (isinstance(nf, LTVZeroPhaseFIRFilter)
                                            and type(nf).forward is LTVZeroPhaseFIRFilter.forward)):
            _refuse(f"the noise filter {type(nf).__name__}")
        ef = decoder.end_filter
        if type(ef) is not LTVMinimumPhaseFilterPrecise:
            _refuse(f"the end filter {type(ef).__name__}"
                    + (" (the frame-wise end filter)" if isinstance(ef, LTVMinimumPhaseFilter) else ""))
        rf = decoder.room_filter
        if not (type(rf) is PassThrough or (isinstance(rf, LTIAcousticFilter) and type(rf).forward is LTIAcousticFilter.forward)):
            _refuse(f"the room filter {type(rf).__name__}")
        if int(batch_size) < 1:
            raise ValueError(f"DecoderStream: batch_size={batch_size}")
        self.decoder = decoder
        self.B = int(batch_size)
        self.generated_noise = isinstance(gen, StandardNormalNoise)
        self.has_fir = type(nf) is not PassThrough
        self.has_room = type(rf) is not PassThrough
        self.geometry: Optional[StreamGeometry] = None
        self.finished = False
        self.emitted = 0

    # ---- public -----------------------------------------------------------------------------------------------------------
    @property
    def latency(self) -> int:
        if self.geometry is None:
            raise RuntimeError("DecoderStream.latency: the hops are fixed by the first push")
        return stream_latency(self.geometry)

    def counts(self) -> dict:
        """Steps pushed so far per track (host integers)."""
        return dict(phase=self._ph.end, wsel=self._w.end, noise=None if self.generated_noise else self._noise_pushed,
                    log_mag=self._lm_pushed, gain=self._g.end, a=self._a.end)

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), noise_filter_params: Tuple[AudioTensor, ...] = (),
             end_filter_params: Tuple[AudioTensor, ...] = (), noise: AudioTensor = None, voicing=None,
             **other_params) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("DecoderStream: push after finish()")
        if voicing is not None:
            _refuse("voicing")
        if len(noise_generator_params):
            _refuse("noise generator parameters")
        if len(harm_oscillator_params) != 1:
            _refuse(f"{len(harm_oscillator_params)} oscillator parameters (phase offsets)")
        if len(end_filter_params) != 2 or len(noise_filter_params) != (1 if self.has_fir else 0):
            raise ValueError("DecoderStream.push: end_filter_params=(gain, a) and noise_filter_params=(log_mag,) (or () "
                             "without a noise filter) are required")
        wsel, (gain, a) = harm_oscillator_params[0], end_filter_params
        lm = noise_filter_params[0] if self.has_fir else None
        tracks = [phase, wsel, gain, a] + ([lm] if lm is not None else []) + ([noise] if noise is not None else [])
        if torch.is_grad_enabled() and any(t.requires_grad for t in tracks):
            _refuse("an input that requires grad (streaming is inference only)")
        if noise is None and not self.generated_noise:
            raise ValueError(f"DecoderStream.push: the noise generator {type(self.decoder.noise_generator).__name__} cannot "
                             "run block by block: pass noise= with every push")
        if self.geometry is None:
            self._setup(phase, wsel, gain, a, lm, noise)
        self._check_hops(phase, wsel, gain, a, lm, noise)
        with torch.no_grad():
            self._append(phase, wsel, gain, a, lm, noise)
            return self._advance(final=False)

    def finish(self) -> torch.Tensor:
        """The inputs have ended: the remaining samples, edges as the one-shot call treats them."""
        if self.finished:
            raise RuntimeError("DecoderStream: finish() twice")
        self.finished = True
        if self.geometry is None:
            return torch.empty(self.B, 0)
        with torch.no_grad():
            return self._advance(final=True)

    # ---- set-up -----------------------------------------------------------------------------------------------------------
    def _setup(self, phase, wsel, gain, a, lm, noise):
        if phase.device.type != "cuda":
            raise _lib.GolfError("DecoderStream: golf_amd kernels need ROCm device tensors; there is no CPU path")
        if int(gain.hop_length) != int(a.hop_length):
            raise ValueError(f"DecoderStream: gain at hop {gain.hop_length}, a at hop {a.hop_length}")
        self.M = int(a.shape[2])
        self.geometry = self._source_geometry(phase, wsel, a, lm)
        self._setup_source(phase, lm, noise, self.decoder.room_filter)
        # end filter: y[<0] = 0; the last block is kept for the utterance's final sample (see _tail)
        self._state = torch.zeros(self.B, self.M, device=phase.device)
        self._last_block = None

    # ---- the pipeline -----------------------------------------------------------------------------------------------------
    def _advance(self, final: bool) -> torch.Tensor:
        g = self.geometry
        n_phase, n_wsel = self._ph.end, self._w.end
        if final:
            fl = final_lengths(g, n_phase, self._noise_pushed, self._lm_pushed, min(self._g.end, self._a.end))
            if self._g.end != self._a.end:
                raise ValueError(f"DecoderStream.finish: {self._g.end} gain frames but {self._a.end} coefficient frames")
            n_osc, n_noise, n_nz, E = fl["osc"], fl["noise"], fl["noise_filter"], fl["out"]
            if n_phase >= 1 and n_wsel < 1:
                raise ValueError("DecoderStream.finish: no table-select frame was pushed")
        else:
            n_noise = _noise_available(g, n_phase, self._noise_pushed)
            n_osc = _osc_outputs(g, _osc_segments(g, n_phase, n_wsel) * g.P)
            n_nz = _fir_frames(g, n_noise, self._lm_pushed) * g.fir_hop if self.has_fir else n_noise
            E = emit_count(g, n_phase, n_wsel, self._noise_pushed, self._lm_pushed, self._g.end, self._a.end)
        self._run_oscillator(n_osc, final)
        self._run_noise(n_noise, n_nz, final)
        if E <= self.emitted:
            return torch.empty(self.B, 0, device=self._dev)
        y = self._run_end_filter(E, final)
        out = self._run_room(y)
        self._osc.drop_before(E)
        self._nz.drop_before(E)
        self.emitted = E
        return out

    def _run_end_filter(self, E: int, final: bool) -> torch.Tensor:
        g = self.geometry
        lo = self.emitted
        src = self._osc.get(lo, E) + self._nz.get(lo, E)
        f0 = lo // g.hop
        f1 = min(self._g.end - 1, (E - 1) // g.hop + 1)
        if final and f1 == f0 and self._last_block is not None:
            # the utterance's last sample alone in its frame: its interpolation runs between the last two frames, which only
            # the block before spans -- run that block again from its saved state, one sample longer, and keep that sample
            state, src0, b_lo = self._last_block
            f0 = b_lo // g.hop
            st = state.clone()
            y = GF.ltv_allpole_ss_state(torch.cat([src0, src], 1), self._g.get(f0, f1 + 1), self._a.get(f0, f1 + 1), g.hop, st)
            return y[:, src0.shape[1]:]
        self._last_block = (self._state.clone(), src, lo)
        y = GF.ltv_allpole_ss_state(src, self._g.get(f0, f1 + 1), self._a.get(f0, f1 + 1), g.hop, self._state)
        self._g.drop_before(f0)   # (the frames of this block stay for _last_block)
        self._a.drop_before(f0)
        return y



def _refuse_framewise(what: str):
    raise NotImplementedError(f"FramewiseDecoderStream: {what} is not supported (frame-wise streaming covers golf-ff -- "
                              "SourceFilterSynth with an indexed glottal table, standard normal noise, the zero-phase FIR noise "
                              "filter or none, the centred frame-wise end filter LTVMinimumPhaseFilter, the LTI room filter or "
                              "none -- and golf-v1 -- HarmonicPlusNoiseSynth with an indexed glottal table, the centred "
                              "frame-wise filter on it, the zero-phase FIR noise filter or none, the LTI room filter or none)")


class FramewiseDecoderStream(_SourceStages):
    """Block-by-block synthesis with a decoder built on the frame-wise LPC filter (module docstring):

      golf-ff  ``SourceFilterSynth`` with ``LTVMinimumPhaseFilter(centred=True)`` as its end filter:
               ``push(phase, harm_oscillator_params=(wsel,), noise_filter_params=(log_mag,), end_filter_params=(gain, a),
               noise=None)``
      golf-v1  ``HarmonicPlusNoiseSynth`` with an indexed glottal table, the frame-wise filter as ``harm_filter``, the zero-phase
               FIR or PassThrough as ``noise_filter`` and LTIAcousticFilter or PassThrough as ``end_filter``:
               ``push(phase, harm_oscillator_params=(wsel,), harm_filter_params=(gain, a), noise_filter_params=(log_mag,),
               noise=None)``; the two branches are summed over the shorter one's length, as the one-shot does.

    Same contract as ``DecoderStream``: each push takes the next slice of every track and returns the (B, n) fp32 samples the
    inputs pushed so far determine (``emit_count``), ``finish()`` the rest; ``latency`` and ``counts()`` as there.  Every
    frame of the filter is filtered once, by golf_lti_frames_ola_stream_f32, which carries the last ceil(W/hop) - 1 of them.
    Inference only; one stream for the whole batch."""

    def __init__(self, decoder, batch_size: int):
        from .ctrl import PassThrough
        from .filters import LTIAcousticFilter, LTVMinimumPhaseFilter, LTVZeroPhaseFIRFilter
        from .noise import NoiseBand, SignFlipNoise, StandardNormalNoise, UniformNoise
        from .sf import HarmonicPlusNoiseSynth, SourceFilterSynth
        from .synth import IndexedGlottalFlowTable

        if isinstance(decoder, SourceFilterSynth) and type(decoder).forward is SourceFilterSynth.forward:
            self.hpn = False
            if decoder.subtract_harmonics:
                _refuse_framewise("subtract_harmonics=True")
            lpc, rf, role = decoder.end_filter, decoder.room_filter, "end filter"
        elif isinstance(decoder, HarmonicPlusNoiseSynth) and type(decoder).forward is HarmonicPlusNoiseSynth.forward:
            self.hpn = True
            lpc, rf, role = decoder.harm_filter, decoder.end_filter, "harmonic filter"
        else:
            _refuse_framewise(type(decoder).__name__)
        osc = decoder.harm_oscillator
        if not isinstance(osc, IndexedGlottalFlowTable) or type(osc).forward is not IndexedGlottalFlowTable.forward:
            _refuse_framewise(f"the oscillator {type(osc).__name__}")
        gen = decoder.noise_generator
        if isinstance(gen, (UniformNoise, SignFlipNoise, NoiseBand)) or getattr(gen, "uses_reference_values", True):
            _refuse_framewise(f"the noise generator {type(gen).__name__}")
        nf = decoder.noise_filter
        if not (type(nf) is PassThrough or (isinstance(nf, LTVZeroPhaseFIRFilter)
                                            and type(nf).forward is LTVZeroPhaseFIRFilter.forward)):
            _refuse_framewise(f"the noise filter {type(nf).__name__}")
        if type(lpc) is not LTVMinimumPhaseFilter:
            _refuse_framewise(f"the {role} {type(lpc).__name__}")
        if not lpc.centred:
            _refuse_framewise("the frame-wise filter with centred=False")
        if not (type(rf) is PassThrough or (isinstance(rf, LTIAcousticFilter) and type(rf).forward is LTIAcousticFilter.forward)):
            _refuse_framewise(f"the room filter {type(rf).__name__}")
        if int(batch_size) < 1:
            raise ValueError(f"FramewiseDecoderStream: batch_size={batch_size}")
        self.decoder = decoder
        self.B = int(batch_size)
        self.generated_noise = isinstance(gen, StandardNormalNoise)
        self.has_fir = type(nf) is not PassThrough
        self.has_room = type(rf) is not PassThrough
        self._lpc, self._room = lpc, rf
        self.geometry: Optional[StreamGeometry] = None
        self.finished = False
        self.emitted = 0

    # ---- public -----------------------------------------------------------------------------------------------------------
    @property
    def latency(self) -> int:
        if self.geometry is None:
            raise RuntimeError("FramewiseDecoderStream.latency: the hops are fixed by the first push")
        return stream_latency(self.geometry)

    def counts(self) -> dict:
        """Steps pushed so far per track (host integers)."""
        return dict(phase=self._ph.end, wsel=self._w.end, noise=None if self.generated_noise else self._noise_pushed,
                    log_mag=self._lm_pushed, gain=self._g.end, a=self._a.end)

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), noise_filter_params: Tuple[AudioTensor, ...] = (),
             end_filter_params: Tuple[AudioTensor, ...] = (), harm_filter_params: Tuple[AudioTensor, ...] = (),
             noise: AudioTensor = None, voicing=None, **other_params) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("FramewiseDecoderStream: push after finish()")
        if voicing is not None:
            _refuse_framewise("voicing")
        if len(noise_generator_params):
            _refuse_framewise("noise generator parameters")
        if len(harm_oscillator_params) != 1:
            _refuse_framewise(f"{len(harm_oscillator_params)} oscillator parameters (phase offsets)")
        lpc_params, other = (harm_filter_params, end_filter_params) if self.hpn else (end_filter_params, harm_filter_params)
        name = "harm_filter_params" if self.hpn else "end_filter_params"
        if len(lpc_params) != 2 or len(other) or len(noise_filter_params) != (1 if self.has_fir else 0):
            raise ValueError(f"FramewiseDecoderStream.push: {name}=(gain, a) and noise_filter_params=(log_mag,) (or () "
                             "without a noise filter) are required")
        wsel, (gain, a) = harm_oscillator_params[0], lpc_params
        lm = noise_filter_params[0] if self.has_fir else None
        tracks = [phase, wsel, gain, a] + ([lm] if lm is not None else []) + ([noise] if noise is not None else [])
        if torch.is_grad_enabled() and any(t.requires_grad for t in tracks):
            _refuse_framewise("an input that requires grad (streaming is inference only)")
        if noise is None and not self.generated_noise:
            raise ValueError(f"FramewiseDecoderStream.push: the noise generator {type(self.decoder.noise_generator).__name__} "
                             "cannot run block by block: pass noise= with every push")
        if self.geometry is None:
            self._setup(phase, wsel, gain, a, lm, noise)
        self._check_hops(phase, wsel, gain, a, lm, noise)
        with torch.no_grad():
            self._append(phase, wsel, gain, a, lm, noise)
            return self._advance(final=False)

    def finish(self) -> torch.Tensor:
        """The inputs have ended: the remaining samples, edges as the one-shot call treats them."""
        if self.finished:
            raise RuntimeError("FramewiseDecoderStream: finish() twice")
        self.finished = True
        if self.geometry is None:
            return torch.empty(self.B, 0)
        with torch.no_grad():
            return self._advance(final=True)

    # ---- set-up -----------------------------------------------------------------------------------------------------------
    def _setup(self, phase, wsel, gain, a, lm, noise):
        dev = phase.device
        if dev.type != "cuda":
            raise _lib.GolfError("FramewiseDecoderStream: golf_amd kernels need ROCm device tensors; there is no CPU path")
        if int(gain.hop_length) != int(a.hop_length):
            raise ValueError(f"FramewiseDecoderStream: gain at hop {gain.hop_length}, a at hop {a.hop_length}")
        W = int(self._lpc._window.numel())
        if W < 2 * int(a.hop_length):
            raise ValueError(f"FramewiseDecoderStream: window {W} < 2*hop {2 * int(a.hop_length)}")
        self.M = int(a.shape[2])
        self.geometry = self._source_geometry(phase, wsel, a, lm, window=W, hpn=self.hpn)
        self._setup_source(phase, lm, noise, self._room)
        # the frame-wise filter: its input x (global samples), frames filtered, output samples written, the carried frames
        self._window = self._lpc._window.detach().float().to(dev).contiguous()
        self._x = _Track()
        self._frames = 0
        self._filtered = 0
        self._carry = None
        self._harm = _Track()   # golf-v1: the filtered oscillator ahead of the filtered noise

    # ---- the pipeline -----------------------------------------------------------------------------------------------------
    def _advance(self, final: bool) -> torch.Tensor:
        g = self.geometry
        n_phase, n_wsel = self._ph.end, self._w.end
        if final:
            if self._g.end != self._a.end:
                raise ValueError(f"FramewiseDecoderStream.finish: {self._g.end} gain frames but {self._a.end} coefficient "
                                 "frames")
            if n_phase >= 1 and n_wsel < 1:
                raise ValueError("FramewiseDecoderStream.finish: no table-select frame was pushed")
            fl = final_lengths(g, n_phase, self._noise_pushed, self._lm_pushed, self._g.end)
            n_osc, n_noise, n_nz = fl["osc"], fl["noise"], fl["noise_filter"]
            n_x, nfr, n_y, E = fl["filter_in"], fl["frames"], fl["filter_out"], fl["out"]
        else:
            n_noise = _noise_available(g, n_phase, self._noise_pushed)
            n_osc = _osc_outputs(g, _osc_segments(g, n_phase, n_wsel) * g.P)
            n_nz = _fir_frames(g, n_noise, self._lm_pushed) * g.fir_hop if self.has_fir else n_noise
            E, nfr, n_y, n_x = _ff_emit(g, n_phase, n_wsel, self._noise_pushed, self._lm_pushed, self._g.end, self._a.end)
        self._run_oscillator(n_osc, final)
        self._run_noise(n_noise, n_nz, final)
        y = self._run_frame_filter(n_x, nfr, n_y, final)
        if g.hpn:
            self._harm.append(y)   # (ahead of the filtered noise: kept until the sum reaches it)
        if E <= self.emitted:
            return torch.empty(self.B, 0, device=self._dev)
        if g.hpn:
            out = self._harm.get(self.emitted, E) + self._nz.get(self.emitted, E)
            self._harm.drop_before(E)
            self._nz.drop_before(E)
        else:
            out = y
        out = self._run_room(out)
        self.emitted = E
        return out

    def _run_frame_filter(self, n_x: int, nfr: int, n_y: int, final: bool) -> torch.Tensor:
        """Extend the filter's input to n_x samples, filter frames up to nfr and write its samples up to n_y."""
        g = self.geometry
        if n_x > self._x.end:
            lo = self._x.end
            x = self._osc.get(lo, n_x) if g.hpn else self._osc.get(lo, n_x) + self._nz.get(lo, n_x)
            self._x.append(x)
            self._osc.drop_before(n_x)
            if not g.hpn:
                self._nz.drop_before(n_x)
        f0, n0 = self._frames, self._filtered
        if nfr <= f0 and n_y <= n0:
            return torch.empty(self.B, 0, device=self._dev)
        empty = lambda *s: torch.empty(self.B, *s, device=self._dev)
        y, self._carry = GF.lti_frames_ola_stream(
            self._x.data if self._x.data is not None else empty(0), self._g.data if self._g.data is not None else empty(0),
            self._a.data if self._a.data is not None else empty(0, self.M), self._window, g.hop, self._carry,
            x0=self._x.start, g0=self._g.start, a0=self._a.start, f0=f0, nf=max(0, nfr - f0), n0=n0, ny=max(0, n_y - n0),
            x_end=n_x if final else -1, g_end=self._g.end if final else -1)
        self._frames, self._filtered = max(f0, nfr), max(n0, n_y)
        t_next = max(0, self._frames * g.hop - g.pad)   # the first sample the next frame reads
        self._x.drop_before(t_next)
        self._g.drop_before(t_next // g.hop)
        self._a.drop_before(self._frames)
        return y


# ---- harmonic-plus-noise decoders ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BranchGeometry:
    """One branch filter of a harmonic-plus-noise decoder (the harmonic or the noise branch)."""
    kind: str = "pass"     # "pass" (PassThrough) | "fir" (LTVZeroPhaseFIRFilter) | "frames" (LTVMinimumPhaseFilter)
    hop: int = 1           # hop of its controls: the log magnitudes, or gain / a
    taps: int = 0          # fir: N = 2*(n_mag-1)
    window: int = 0        # frames: W
    centred: bool = True   # frames: False shifts the input by hop//2 and reflect-pads the output by as much

    @property
    def shift(self) -> int:   # hop//2 of centred=False
        return 0 if self.kind != "frames" or self.centred else self.hop // 2


@dataclass(frozen=True)
class HPNGeometry:
    """What the bookkeeping of ``HarmonicPlusNoiseStream`` depends on.  Hops are in output samples."""
    phase_hop: int
    source: str = "harmonic"   # "harmonic" (golf_harmonic_osc_stream_f32) | "glottal" (golf_glottal_osc_stream_f32)
    amp_hop: int = 0           # harmonic: hop of the amplitude rows; 0: no amplitude track
    os: int = 1                # glottal: oversampling, decimator half width, table-select hop
    half: int = 0
    w_hop: int = 1
    harm: BranchGeometry = field(default_factory=BranchGeometry)
    noise: BranchGeometry = field(default_factory=BranchGeometry)

    @property
    def glottal(self) -> StreamGeometry:
        return StreamGeometry(hop=1, phase_hop=self.phase_hop, os=self.os, half=self.half, w_hop=self.w_hop)


def _up_len(n: int, hop: int) -> int:
    return 0 if n < 1 else ((n - 1) * hop + 1 if hop > 1 else n)


def _hpn_source_open(g: HPNGeometry, n_phase: int, n_src: Optional[int]) -> Tuple[int, int]:
    """(segments, samples) of the source that can be rendered while the inputs are open: segment j needs p[j+1] and, for its
    last sample, the amplitude row after the one it sits in (glottal: ``_osc_segments``)."""
    if g.source == "glottal":
        nseg = _osc_segments(g.glottal, n_phase, n_src)
        return nseg, _osc_outputs(g.glottal, nseg * g.glottal.P)
    nseg = max(0, n_phase - 1)
    if g.amp_hop:
        nseg = min(nseg, max(0, (n_src - 1) * g.amp_hop) // g.phase_hop)
    return nseg, nseg * g.phase_hop


def _hpn_source_len(g: HPNGeometry, n_phase: int, n_src: Optional[int]) -> int:
    """The one-shot oscillator's length for these counts: final, and a lower bound while the inputs are open."""
    if g.source == "glottal":
        return _osc_len(g.glottal, n_phase)
    n = _up_len(n_phase, g.phase_hop)
    return min(n, _up_len(n_src, g.amp_hop)) if g.amp_hop else n


def _branch_open(b: BranchGeometry, n_in: int, ctrl: Tuple[int, ...]) -> Tuple[int, int, int, int]:
    """(branch outputs finished, frames ready, filter outputs finished, filter inputs known) while the inputs are open, given
    ``n_in`` known input samples and the pushed control rows (fir: (log_mag,), frames: (gain, a))."""
    if b.kind == "pass":
        return n_in, 0, n_in, n_in
    if b.kind == "fir":
        f = max(0, min(ctrl[0], (n_in - (b.taps - 1 - (b.taps - 1) // 2)) // b.hop))
        return f * b.hop, f, f * b.hop, n_in
    pad, n_x = b.window // 2, max(0, n_in - b.shift)
    c = (b.window - pad - 1) // b.hop
    nfr = max(0, min((n_x + pad - b.window) // b.hop + 1, ctrl[1], ctrl[0] - 1 - c))
    n_y = max(0, nfr * b.hop - pad)
    out = n_y if not b.shift else (n_y + b.shift if n_y > b.shift else 0)   # the reflect pad needs y[1 .. shift]
    return out, nfr, n_y, n_x


def _branch_final(b: BranchGeometry, n_in: int, ctrl: Tuple[int, ...]) -> dict:
    """The one-shot branch filter's lengths for an input of ``n_in`` samples: its output (``out``) and, frame-wise, its input
    (``filter_in``, the one-shot's Tx after the shift), frames and filter output."""
    if b.kind == "pass":
        return dict(out=n_in)
    if b.kind == "fir":
        P = (b.taps - 1) // 2
        span = n_in + 2 * P - (b.taps + b.hop - 1)
        if span < 0:
            raise _lib.GolfError(f"HarmonicPlusNoiseStream: {n_in} samples are shorter than one FIR frame span")
        return dict(out=min(span // b.hop + 1, ctrl[0]) * b.hop)
    F = ctrl[0]
    x = n_in - b.shift
    Tx, nfr, Ty = GF.ff_output_length(x, F, b.hop, b.window) if x >= 1 and F >= 2 else (0, 0, 0)
    if nfr > F:
        raise _lib.GolfError(f"frame-wise filter: {nfr} frames needed but only {F} coefficient frames")
    if b.shift and Ty <= b.shift:
        raise _lib.GolfError(f"frame-wise filter (centred=False): {Ty} output samples cannot be reflect-padded by {b.shift}")
    return dict(out=Ty + b.shift, filter_in=Tx, frames=nfr, filter_out=Ty)


def hpn_emit_count(g: HPNGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int], harm_ctrl: Tuple[int, ...],
                   noise_ctrl: Tuple[int, ...]) -> int:
    """E: the output samples [0, E) ``HarmonicPlusNoiseStream`` emits once these many steps of each track have been pushed.
    ``n_phase``: phase steps (with voicing, the steps both tracks have); ``n_src``: amplitude rows (harmonic source; None
    without an amplitude track) or table-select rows (glottal); ``n_noise`` None: the noise is drawn on the device;
    ``harm_ctrl`` / ``noise_ctrl``: each branch's control rows, () / (log_mag,) / (gain, a).  Every sample below E is
    determined by what has been pushed: the source's segments, the noise the one-shot is certain to draw, and each branch's
    stencil; the output is the sum of the two branches over the shorter one."""
    n_osc = _hpn_source_open(g, n_phase, n_src)[1]
    lb = _hpn_source_len(g, n_phase, n_src)
    nz = lb if n_noise is None else min(n_noise, lb)
    return min(_branch_open(g.harm, n_osc, harm_ctrl)[0], _branch_open(g.noise, nz, noise_ctrl)[0])


def hpn_final_lengths(g: HPNGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int], harm_ctrl: Tuple[int, ...],
                      noise_ctrl: Tuple[int, ...]) -> dict:
    """Lengths of the one-shot decoder's stages once the inputs have ended: the oscillator (``source``), the noise, each
    branch (``harm``, ``noise_branch``: dicts of ``_branch_final``) and the output, the shorter branch."""
    src = _hpn_source_len(g, n_phase, n_src)
    noise = src if n_noise is None else min(n_noise, src)
    h = _branch_final(g.harm, src, harm_ctrl)
    n = _branch_final(g.noise, noise, noise_ctrl)
    return dict(source=src, noise=noise, harm=h, noise_branch=n, out=min(h["out"], n["out"]))


def _branch_lookahead(b: BranchGeometry, L_in: int) -> int:
    if b.kind == "pass":
        return L_in
    if b.kind == "fir":
        return b.hop - 1 + (b.taps - 1 - (b.taps - 1) // 2) + L_in
    pad, s = b.window // 2, b.shift
    c = (b.window - pad - 1) // b.hop
    q = max(b.window - 1 + L_in, pad - s + b.hop * (c + 1))
    if s:   # centred=False: outputs 0 .. s-1 wait for output 2s, whose frame f0 reads input up to f0*hop - pad + W - 1 + s
        f0 = (s + pad) // b.hop
        q = max(q, f0 * b.hop - pad + b.window - 1 + s + L_in, b.hop * (f0 + c + 1))
    return q


def hpn_stream_latency(g: HPNGeometry) -> int:
    """Worst-case lookahead of ``HarmonicPlusNoiseStream`` in samples: output sample t is emitted at the latest once every
    track has been pushed up to input time t + latency.  Per stage, the input time past a sample that determines it:
      harmonic source   P + A - gcd(P, A)  (P the phase hop, A the amplitude hop: p[j+1] closes segment j, the segment's last
                        sample needs the amplitude row after its own; P without amplitudes)
      glottal source    as ``stream_latency`` (phase, table select, decimator)
      noise             max(P - 1, A - 1): the samples the one-shot is certain to draw
      FIR branch        + fir_hop - 1 + R  (R = N-1-(N-1)//2 samples read past the one written)
      frame-wise branch max(W - 1 + input, pad - s + hop * ((W - pad - 1) // hop + 1)) + 2 s   (s = hop//2 without centring)
    and the output waits for both branches.  DDSP (phase at hop 1, amplitudes at 240, FIR 510 at 240): 239 + 239 + 255 = 733."""
    if g.source == "glottal" and g.os == 1:   # no decimator: as the harmonic source, the table-select rows as amplitudes
        L_src = g.phase_hop + g.w_hop - math.gcd(g.phase_hop, g.w_hop)
        L_nz = g.phase_hop - 1
    elif g.source == "glottal":
        sg = g.glottal
        L_src = max(sg.phase_hop + sg.half // sg.os, sg.w_hop + (sg.half + sg.P - 1) // sg.os, 1)
        L_nz = g.phase_hop - 1
    else:
        P, A = g.phase_hop, g.amp_hop
        L_src = P + A - math.gcd(P, A) if A else P
        L_nz = max(P - 1, A - 1 if A else 0)
    return max(_branch_lookahead(g.harm, L_src), _branch_lookahead(g.noise, L_nz))


class _BranchStage:
    """One branch filter run block by block.  It reads its input from the upstream track ``src`` (which it alone consumes and
    trims) and appends its finished output samples to ``out`` (global indices; PassThrough: ``out`` is ``src``)."""

    def __init__(self, b: BranchGeometry, module, src: _Track, B: int, dev):
        self.b, self.src, self.B, self._dev = b, src, B, dev
        self.out = src if b.kind == "pass" else _Track()
        self.n_ctrl = 0
        if b.kind == "fir":
            self._kern = _Track()
            self._frames = 0
            self._window = module._window(b.taps, dev)
            self._basis = GF.zero_phase_fir_basis(b.taps // 2 + 1, dev)
        elif b.kind == "frames":
            self._x, self._g, self._a, self._y = _Track(), _Track(), _Track(), _Track()
            self._win = module._window.detach().float().to(dev).contiguous()
            self._frames = self._filtered = 0
            self._carry = None

    def ctrl(self) -> Tuple[int, ...]:
        """The control rows pushed so far: () / (log_mag,) / (gain, a)."""
        if self.b.kind == "fir":
            return (self.n_ctrl,)
        return (self._g.end, self._a.end) if self.b.kind == "frames" else ()

    def append(self, params, f32) -> None:
        if self.b.kind == "fir":
            lm = params[0]
            if lm.shape[1]:
                x = f32(lm).contiguous()
                kern = GF._zp_kernels_raw(_lib.load(), x, self._window, self._basis)
                self._kern.append(kern.view(self.B, x.shape[1], -1))
            self.n_ctrl += lm.shape[1]
        elif self.b.kind == "frames":
            self._g.append(f32(params[0]))
            self._a.append(f32(params[1]).contiguous())

    def run(self, n_in: int, final: bool, fin: Optional[dict]) -> None:
        """The input is known up to ``n_in`` samples (at finish: the one-shot's input length, ``fin`` its lengths)."""
        if self.b.kind == "fir":
            self._run_fir(n_in, final, fin)
        elif self.b.kind == "frames":
            self._run_frames(n_in, final, fin)

    def _run_fir(self, n_in: int, final: bool, fin) -> None:   # (_SourceStages._run_noise on this branch's tracks)
        b = self.b
        f_lo = self._frames
        f_hi = fin["out"] // b.hop if final else _branch_open(b, n_in, self.ctrl())[1]
        if f_hi <= f_lo:
            return
        R = b.taps - 1 - (b.taps - 1) // 2
        q = -(-((b.taps - 1) // 2) // b.hop)          # frames whose left context would be the call's zero padding
        fs = max(0, f_lo - q)
        e = n_in if final else min(n_in, f_hi * b.hop + R)
        x = self.src.get(fs * b.hop, e)
        kern = self._kern.data
        Fk = kern.shape[1]
        y = GF._FIRFrames.apply(x, kern.reshape(self.B * Fk, -1), Fk, b.taps, b.hop, fs - self._kern.start)
        self.out.append(y[:, (f_lo - fs) * b.hop: (f_hi - fs) * b.hop])
        self._frames = f_hi
        nxt = max(0, f_hi - q)
        self.src.drop_before(nxt * b.hop)
        self._kern.drop_before(nxt)

    def _run_frames(self, n_in: int, final: bool, fin) -> None:   # (FramewiseDecoderStream._run_frame_filter, shifted)
        b, s = self.b, self.b.shift
        if final:
            if self._g.end != self._a.end:
                raise ValueError(f"HarmonicPlusNoiseStream.finish: {self._g.end} gain frames but {self._a.end} coefficient "
                                 "frames")
            n_x, nfr, n_y = fin.get("filter_in", 0), fin.get("frames", 0), fin.get("filter_out", 0)
            n_out = fin["out"]
        else:
            n_out, nfr, n_y, n_x = _branch_open(b, n_in, self.ctrl())
        if n_x > self._x.end:
            lo = self._x.end
            self._x.append(self.src.get(lo + s, n_x + s))
            self.src.drop_before(n_x + s)
        f0, n0 = self._frames, self._filtered
        if nfr > f0 or n_y > n0:
            empty = lambda *sh: torch.empty(self.B, *sh, device=self._dev)
            data = lambda t, *sh: t.data if t.data is not None else empty(*sh)
            y, self._carry = GF.lti_frames_ola_stream(
                data(self._x, 0), data(self._g, 0), data(self._a, 0, 1 if self._a.data is None else self._a.data.shape[2]),
                self._win, b.hop, self._carry, x0=self._x.start, g0=self._g.start, a0=self._a.start, f0=f0,
                nf=max(0, nfr - f0), n0=n0, ny=max(0, n_y - n0), x_end=n_x if final else -1,
                g_end=self._g.end if final else -1)
            self._frames, self._filtered = max(f0, nfr), max(n0, n_y)
            t_next = max(0, self._frames * b.hop - b.window // 2)   # the first sample the next frame reads
            self._x.drop_before(t_next)
            self._g.drop_before(t_next // b.hop)
            self._a.drop_before(self._frames)
            if not s:
                self.out.append(y)
                return
            self._y.append(y)
        if s and n_out > self.out.end:
            if self.out.end == 0:   # the one-shot's reflect pad: outputs 0 .. s-1 are filter outputs s .. 1
                self.out.append(self._y.get(1, s + 1).flip(1))
            self.out.append(self._y.get(self.out.end - s, n_out - s))
            self._y.drop_before(n_out - s)


def _refuse_hpn(what: str):
    raise NotImplementedError(f"HarmonicPlusNoiseStream: {what} is not supported (it covers HarmonicPlusNoiseSynth with the "
                              "harmonic oscillator bank -- HarmonicOscillator, AdditiveSynthesizer, V1AdditiveSynthesizer, "
                              "SawToothOscillator, AdditivePulseTrain -- or an indexed glottal table; PassThrough, "
                              "LTVZeroPhaseFIRFilter or LTVMinimumPhaseFilter on each branch; standard normal noise or noise "
                              "pushed with every block; PassThrough or LTIAcousticFilter as the end filter; voicing at the "
                              "phase's hop)")


class HarmonicPlusNoiseStream(_SourceStages):
    """Block-by-block synthesis with a ``HarmonicPlusNoiseSynth`` (module docstring, INTEGRATION.md "Streaming synthesis"):

        ``push(phase, harm_oscillator_params=..., harm_filter_params=..., noise_filter_params=..., noise=None, voicing=None)``

    with the one-shot call's arguments sliced: ``harm_oscillator_params`` (amplitudes,) for HarmonicOscillator,
    AdditiveSynthesizer and V1AdditiveSynthesizer, () for SawToothOscillator and AdditivePulseTrain, (wsel,) for the glottal
    table; each branch's params () / (log_mag,) / (gain, a) for PassThrough / LTVZeroPhaseFIRFilter / LTVMinimumPhaseFilter;
    ``voicing`` (at the phase's hop) multiplies the phase as the one-shot does.  Same contract as ``DecoderStream``: each push
    returns the (B, n) fp32 samples the inputs pushed so far determine (``hpn_emit_count``), ``finish()`` the rest;
    ``latency`` and ``counts()`` as there.  ``open_stream`` does not return this class: open it explicitly.
    Inference only; one stream for the whole batch."""

    def __init__(self, decoder, batch_size: int):
        from .ctrl import PassThrough
        from .filters import LTIAcousticFilter, LTVMinimumPhaseFilter, LTVZeroPhaseFIRFilter
        from .noise import NoiseBand, SignFlipNoise, StandardNormalNoise, UniformNoise
        from .sf import HarmonicPlusNoiseSynth
        from .synth import (AdditivePulseTrain, AdditiveSynthesizer, HarmonicOscillator, IndexedGlottalFlowTable,
                            SawToothOscillator, V1AdditiveSynthesizer)

        if not isinstance(decoder, HarmonicPlusNoiseSynth) or type(decoder).forward is not HarmonicPlusNoiseSynth.forward:
            _refuse_hpn(type(decoder).__name__)
        osc = decoder.harm_oscillator
        if type(osc) in (HarmonicOscillator, AdditiveSynthesizer, V1AdditiveSynthesizer, SawToothOscillator,
                         AdditivePulseTrain):
            self.source = "harmonic"
            self._osc_kind = type(osc)
        elif isinstance(osc, IndexedGlottalFlowTable) and type(osc).forward is IndexedGlottalFlowTable.forward:
            self.source = "glottal"
        else:
            _refuse_hpn(f"the oscillator {type(osc).__name__}")
        gen = decoder.noise_generator
        if isinstance(gen, (UniformNoise, SignFlipNoise, NoiseBand)) or getattr(gen, "uses_reference_values", True):
            _refuse_hpn(f"the noise generator {type(gen).__name__}")
        self._kinds = {}
        for role, f in (("harmonic filter", decoder.harm_filter), ("noise filter", decoder.noise_filter)):
            if type(f) is PassThrough:
                self._kinds[role] = "pass"
            elif isinstance(f, LTVZeroPhaseFIRFilter) and type(f).forward is LTVZeroPhaseFIRFilter.forward:
                self._kinds[role] = "fir"
            elif type(f) is LTVMinimumPhaseFilter:
                self._kinds[role] = "frames"
            else:
                _refuse_hpn(f"the {role} {type(f).__name__}"
                            + (" (the sample-wise LPC filter)" if type(f).__name__ == "LTVMinimumPhaseFilterPrecise" else ""))
        ef = decoder.end_filter
        if not (type(ef) is PassThrough or (isinstance(ef, LTIAcousticFilter) and type(ef).forward is LTIAcousticFilter.forward)):
            _refuse_hpn(f"the end filter {type(ef).__name__}")
        if int(batch_size) < 1:
            raise ValueError(f"HarmonicPlusNoiseStream: batch_size={batch_size}")
        self.decoder = decoder
        self.B = int(batch_size)
        self.generated_noise = isinstance(gen, StandardNormalNoise)
        self.has_room = type(ef) is not PassThrough
        self.geometry: Optional[HPNGeometry] = None
        self.finished = False
        self.emitted = 0

    # ---- public -----------------------------------------------------------------------------------------------------------
    @property
    def latency(self) -> int:
        if self.geometry is None:
            raise RuntimeError("HarmonicPlusNoiseStream.latency: the hops are fixed by the first push")
        return hpn_stream_latency(self.geometry)

    def counts(self) -> dict:
        """Steps pushed so far per track (host integers)."""
        return dict(phase=self._praw.end, voicing=self._vraw.end if self._voiced else None,
                    oscillator=self._src_count(), noise=None if self.generated_noise else self._noise_pushed,
                    harm_filter=self._harm.ctrl(), noise_filter=self._nzb.ctrl())

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), harm_filter_params: Tuple[AudioTensor, ...] = (),
             noise_filter_params: Tuple[AudioTensor, ...] = (), noise: AudioTensor = None, voicing: AudioTensor = None,
             **other_params) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("HarmonicPlusNoiseStream: push after finish()")
        if len(noise_generator_params):
            _refuse_hpn("noise generator parameters")
        n_osc = 1 if self.source == "glottal" or self._amp_track() else 0
        if len(harm_oscillator_params) != n_osc:
            _refuse_hpn(f"{len(harm_oscillator_params)} oscillator parameters for {type(self.decoder.harm_oscillator).__name__}"
                        f" (it takes {n_osc}; initial_phase / phase_offset are not streamed)")
        want = {"pass": 0, "fir": 1, "frames": 2}
        for name, params, role in (("harm_filter_params", harm_filter_params, "harmonic filter"),
                                   ("noise_filter_params", noise_filter_params, "noise filter")):
            if len(params) != want[self._kinds[role]]:
                raise ValueError(f"HarmonicPlusNoiseStream.push: {name} must hold {want[self._kinds[role]]} tracks for the "
                                 f"{role} ({self._kinds[role]})")
        tracks = [phase, *harm_oscillator_params, *harm_filter_params, *noise_filter_params] + \
            [t for t in (noise, voicing) if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in tracks):
            _refuse_hpn("an input that requires grad (streaming is inference only)")
        if noise is None and not self.generated_noise:
            raise ValueError(f"HarmonicPlusNoiseStream.push: the noise generator {type(self.decoder.noise_generator).__name__}"
                             " cannot run block by block: pass noise= with every push")
        if voicing is not None and int(voicing.hop_length) != int(phase.hop_length):
            _refuse_hpn(f"voicing at hop {voicing.hop_length} with the phase at hop {phase.hop_length}")
        if self.geometry is None:
            self._setup(phase, harm_oscillator_params, harm_filter_params, noise_filter_params, noise, voicing)
        self._check(phase, harm_oscillator_params, harm_filter_params, noise_filter_params, noise, voicing)
        with torch.no_grad():
            self._append(phase, harm_oscillator_params, harm_filter_params, noise_filter_params, noise, voicing)
            return self._advance(final=False)

    def finish(self) -> torch.Tensor:
        """The inputs have ended: the remaining samples, edges as the one-shot call treats them."""
        if self.finished:
            raise RuntimeError("HarmonicPlusNoiseStream: finish() twice")
        self.finished = True
        if self.geometry is None:
            return torch.empty(self.B, 0)
        with torch.no_grad():
            return self._advance(final=True)

    # ---- set-up -----------------------------------------------------------------------------------------------------------
    def _amp_track(self) -> bool:
        from .synth import AdditivePulseTrain, SawToothOscillator

        return self.source == "harmonic" and self._osc_kind not in (SawToothOscillator, AdditivePulseTrain)

    def _setup(self, phase, osc_params, hf_params, nf_params, noise, voicing):
        from .synth import AdditivePulseTrain, AdditiveSynthesizer, SawToothOscillator

        dev = phase.device
        dec, P = self.decoder, int(phase.hop_length)
        branches = {}
        for role, f, params in (("harmonic filter", dec.harm_filter, hf_params), ("noise filter", dec.noise_filter, nf_params)):
            kind = self._kinds[role]
            if kind == "fir":
                branches[role] = BranchGeometry("fir", hop=int(params[0].hop_length), taps=2 * (int(params[0].shape[2]) - 1))
            elif kind == "frames":
                if int(params[0].hop_length) != int(params[1].hop_length):
                    raise ValueError(f"HarmonicPlusNoiseStream: {role} gain at hop {params[0].hop_length}, a at hop "
                                     f"{params[1].hop_length}")
                hop, W = int(params[1].hop_length), int(f._window.numel())
                if W < 2 * hop:
                    raise ValueError(f"HarmonicPlusNoiseStream: {role} window {W} < 2*hop {2 * hop}")
                branches[role] = BranchGeometry("frames", hop=hop, window=W, centred=bool(f.centred))
            else:
                branches[role] = BranchGeometry()
        osc = dec.harm_oscillator
        self._ts_mode = None
        if self.source == "glottal":
            wsel = osc_params[0]
            self._source_geometry(phase, wsel, wsel, None)   # (sets the table and the decimator taps)
            g = HPNGeometry(phase_hop=P, source="glottal", os=int(osc.oversampling),
                            half=(self._taps.numel() - 1) // 2 if self._taps is not None else 0, w_hop=int(wsel.hop_length),
                            harm=branches["harmonic filter"], noise=branches["noise filter"])
            self._w = _Track()
            self._pre = None
        else:
            A = 0
            if self._amp_track():
                A = int(osc_params[0].hop_length)
                if self._osc_kind is AdditiveSynthesizer and P != 1:
                    if A != P:
                        _refuse_hpn(f"AdditiveSynthesizer with the phase at hop {P} and the amplitudes at hop {A} (the phase "
                                    "hop must be 1 or the amplitude hop)")
                    self._ts_mode = "fold"
                elif self._osc_kind is AdditiveSynthesizer:
                    self._ts_mode = "phase"
                if P > 1 and A % P:
                    _refuse_hpn(f"amplitudes at hop {A} with the phase at hop {P} (a multiple of the phase hop is needed)")
                self.H = int(osc_params[0].shape[2])
            elif self._osc_kind is SawToothOscillator:
                self.H = int(osc.amplitudes.numel())
            else:
                self.H = int(osc.num_harmonics)
            if self._osc_kind is AdditivePulseTrain:
                self._ts_mode = "phase"
            self._hscale = osc.amplitudes.detach().float().to(dev).contiguous() if self._osc_kind is SawToothOscillator else None
            g = HPNGeometry(phase_hop=P, source="harmonic", amp_hop=A, harm=branches["harmonic filter"],
                            noise=branches["noise filter"])
            self._amp, self._araw, self._sc = _Track(), _Track(), _Track()
        if dev.type != "cuda":
            raise _lib.GolfError("HarmonicPlusNoiseStream: golf_amd kernels need ROCm device tensors; there is no CPU path")
        self._dev = dev
        if self.source == "glottal":
            pad = -(-g.half // g.os) * g.os   # zeros before fine sample 0: the one-shot decimator's own zero padding
            self._pre = _Track(-pad, torch.zeros(self.B, pad, device=dev))
        self.geometry = g
        self._voiced = voicing is not None
        self._praw, self._vraw, self._ph = _Track(), _Track(), _Track()
        self._seg = 0
        self._acc = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self._osc, self._noise = _Track(), _Track()
        self._noise_pushed = None if noise is None else 0
        self._harm = _BranchStage(g.harm, dec.harm_filter, self._osc, self.B, dev)
        self._nzb = _BranchStage(g.noise, dec.noise_filter, self._noise, self.B, dev)
        if self.has_room:
            room = dec.end_filter
            self._room_lead = room._padding
            self._room_taps = torch.cat([room.kernel.detach(), room._tail.to(room.kernel.dtype)]).float().contiguous()
            self._room_hist = torch.zeros(self.B, self._room_lead, device=dev)

    def _check(self, phase, osc_params, hf_params, nf_params, noise, voicing):
        g = self.geometry
        want = [(phase, g.phase_hop, "phase")]
        if voicing is not None:
            want.append((voicing, g.phase_hop, "voicing"))
        if self.source == "glottal":
            want.append((osc_params[0], g.w_hop, "table select"))
        elif g.amp_hop:
            want.append((osc_params[0], g.amp_hop, "amplitudes"))
        for b, params, role in ((g.harm, hf_params, "harmonic filter"), (g.noise, nf_params, "noise filter")):
            want += [(t, b.hop, f"{role} track") for t in params]
        if noise is not None:
            want.append((noise, 1, "noise"))
        for t, hop, name in want:
            if int(t.hop_length) != hop or t.shape[0] != self.B:
                raise ValueError(f"HarmonicPlusNoiseStream.push: {name} of shape {tuple(t.shape)} at hop {t.hop_length}; "
                                 f"the stream has B={self.B}, hop {hop}")
        if self._amp_track() and int(osc_params[0].shape[2]) != self.H:
            raise ValueError("HarmonicPlusNoiseStream.push: the number of harmonics changed between pushes")
        for b, params in ((g.harm, hf_params), (g.noise, nf_params)):
            if b.kind == "fir" and 2 * (int(params[0].shape[2]) - 1) != b.taps:
                raise ValueError("HarmonicPlusNoiseStream.push: the FIR bins changed between pushes")
        if (noise is None) != (self._noise_pushed is None):
            raise ValueError("HarmonicPlusNoiseStream.push: pass noise= in every push or in none")
        if (voicing is None) == self._voiced:
            raise ValueError("HarmonicPlusNoiseStream.push: pass voicing= in every push or in none")

    def _append(self, phase, osc_params, hf_params, nf_params, noise, voicing):
        # (autocast: fp16 / bf16 control tracks become fp32 here, before any kernel sees them)
        f32 = lambda t: t.as_tensor().to(device=self._dev, dtype=torch.float32)
        self._praw.append(f32(phase))
        if voicing is not None:
            self._vraw.append(f32(voicing))
        n = min(self._praw.end, self._vraw.end) if self._voiced else self._praw.end
        if n > self._ph.end:   # the phase the oscillator sees: phase * voicing, as HarmonicPlusNoiseSynth.forward forms it
            lo = self._ph.end
            p = self._praw.get(lo, n) * self._vraw.get(lo, n) if self._voiced else self._praw.get(lo, n)
            self._ph.append(p)
            self._praw.drop_before(n)
            self._vraw.drop_before(n)
            if self._ts_mode is not None:   # rsqrt(0.5 / phase): the equal-energy factor (synth.py _sqrt_two_phase)
                self._sc.append(torch.rsqrt(0.5 / p))
        if self.source == "glottal":
            self._w.append(f32(osc_params[0]))
        elif self._amp_track():
            if self._ts_mode == "fold":   # amplitudes * unsqueeze(scale, -1), row by row as both arrive
                self._araw.append(f32(osc_params[0]))
                m = min(self._araw.end, self._sc.end)
                if m > self._amp.end:
                    lo = self._amp.end
                    self._amp.append(self._araw.get(lo, m) * torch.unsqueeze(self._sc.get(lo, m), -1))
                    self._araw.drop_before(m)
                    self._sc.drop_before(m)
            else:
                self._amp.append(f32(osc_params[0]))
        if noise is not None:
            x = f32(noise)
            self._noise.append(x)
            self._noise_pushed += x.shape[1]
        self._harm.append(hf_params, f32)
        self._nzb.append(nf_params, f32)

    def _src_count(self) -> Optional[int]:
        if self.source == "glottal":
            return self._w.end
        return self._amp.end if self.geometry.amp_hop else None

    # ---- the pipeline -----------------------------------------------------------------------------------------------------
    def _advance(self, final: bool) -> torch.Tensor:
        g = self.geometry
        n_phase, n_src = self._ph.end, self._src_count()
        hc, nc = self._harm.ctrl(), self._nzb.ctrl()
        if final:
            if self.source == "glottal" and n_phase >= 1 and n_src < 1:
                raise ValueError("HarmonicPlusNoiseStream.finish: no table-select frame was pushed")
            fl = hpn_final_lengths(g, n_phase, n_src, self._noise_pushed, hc, nc)
            n_osc, n_noise, E = fl["source"], fl["noise"], fl["out"]
            nseg = (n_osc - 1) // g.phase_hop if n_osc else 0
        else:
            fl = None
            nseg, n_osc = _hpn_source_open(g, n_phase, n_src)
            lb = _hpn_source_len(g, n_phase, n_src)
            n_noise = lb if self._noise_pushed is None else min(self._noise_pushed, lb)
            E = hpn_emit_count(g, n_phase, n_src, self._noise_pushed, hc, nc)
        if self.source == "glottal":
            self._run_oscillator(n_osc, final, g.glottal)
        else:
            self._run_harmonic(nseg, final and n_osc >= 1)
        if self.generated_noise and n_noise > self._noise.end:
            self._noise.append(torch.randn(self.B, n_noise - self._noise.end, device=self._dev))
        self._harm.run(n_osc, final, fl["harm"] if final else None)
        self._nzb.run(n_noise, final, fl["noise_branch"] if final else None)
        if E <= self.emitted:
            return torch.empty(self.B, 0, device=self._dev)
        out = self._harm.out.get(self.emitted, E) + self._nzb.out.get(self.emitted, E)
        self._harm.out.drop_before(E)
        self._nzb.out.drop_before(E)
        out = self._run_room(out)
        self.emitted = E
        return out

    def _run_harmonic(self, nseg: int, last: bool) -> None:
        """Render segments [self._seg, nseg) (+ with ``last`` the sample k = 0 of segment nseg: the one-shot's last sample)."""
        g = self.geometry
        if nseg <= self._seg and not last:
            return
        j0, P = self._seg, g.phase_hop
        n = (nseg - j0) * P + int(last)
        t_lo, t_hi = j0 * P, j0 * P + n - 1
        kw = {}
        if g.amp_hop:
            end = self._amp.end if last else -1
            row = lambda t: min(t // g.amp_hop, end - 2) if end >= 2 else (0 if end == 1 else t // g.amp_hop)
            r_lo, r_hi = row(t_lo), min(self._amp.end, row(t_hi) + 2)
            kw.update(amp=self._amp.get(r_lo, r_hi), a_first=r_lo, a_end=end, amp_hop=g.amp_hop)
        if self._ts_mode == "phase":   # tscale rows are the phase rows
            kw.update(tscale=self._sc.get(self._sc.start, self._sc.end), s_first=self._sc.start,
                      s_end=self._sc.end if last else -1, ts_hop=P)
        y = GF.harmonic_osc_stream(self._ph.get(j0, nseg + 1), j0, nseg - j0, last, P, self.H, self._acc,
                                   hscale=self._hscale, **kw)
        self._osc.append(y)
        self._seg = nseg
        self._ph.drop_before(nseg)        # p[nseg] closes the next segment
        # rows the next call reads: from the next sample's row on, and the last two (the end clamp interpolates between them)
        if g.amp_hop:
            self._amp.drop_before(min((nseg * P) // g.amp_hop, self._amp.end - 2))
        if self._ts_mode == "phase":
            self._sc.drop_before(min(nseg, self._sc.end - 2))


def open_stream(decoder, batch_size: int):
    """A streaming synthesiser for ``decoder``: ``FramewiseDecoderStream`` for the decoders built on the frame-wise LPC filter
    (golf-ff's end filter, golf-v1's harmonic filter), ``DecoderStream`` otherwise (golf-ss)."""
    from .filters import LTVMinimumPhaseFilter
    from .sf import HarmonicPlusNoiseSynth

    if isinstance(decoder, HarmonicPlusNoiseSynth) or isinstance(getattr(decoder, "end_filter", None), LTVMinimumPhaseFilter):
        return FramewiseDecoderStream(decoder, batch_size)
    return DecoderStream(decoder, batch_size)
