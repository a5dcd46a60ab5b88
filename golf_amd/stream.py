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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["DecoderStream", "FramewiseDecoderStream", "StreamGeometry", "emit_count", "final_lengths", "open_stream",
           "stream_latency"]


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

    def _run_oscillator(self, n_osc: int, final: bool) -> None:
        g = self.geometry
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


def open_stream(decoder, batch_size: int):
    """A streaming synthesiser for ``decoder``: ``FramewiseDecoderStream`` for the decoders built on the frame-wise LPC filter
    (golf-ff's end filter, golf-v1's harmonic filter), ``DecoderStream`` otherwise (golf-ss)."""
    from .filters import LTVMinimumPhaseFilter
    from .sf import HarmonicPlusNoiseSynth

    if isinstance(decoder, HarmonicPlusNoiseSynth) or isinstance(getattr(decoder, "end_filter", None), LTVMinimumPhaseFilter):
        return FramewiseDecoderStream(decoder, batch_size)
    return DecoderStream(decoder, batch_size)
