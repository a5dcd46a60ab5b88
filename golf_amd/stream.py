"""Streaming GOLF synthesis: the decoder fed control frames as they are produced, audio returned block by block.

Every ``push`` of a stream hands over the NEXT slice of each input track (any length, 0 included) and returns the output samples
that the inputs pushed so far determine; ``finish()`` returns the rest, with the utterance's edges treated exactly as the
one-shot call treats them.  The concatenation of all outputs is ``decoder(...)`` on the concatenated inputs (INTEGRATION.md
"Streaming synthesis").

The streams are built from one set of stages.  A stage owns its tracks and what it carries across a block boundary, and its
``run`` extends its output track:
  _GlottalSource    the exact Q0.64 phase accumulator (golf_glottal_osc_stream_f32) and the last (K-1)/2 fine samples of the
                    decimator's context (golf_decimate_fir_f32 over an overlap window)
  _HarmonicSource   the oscillator bank from a carried Q0.64 phase (golf_harmonic_osc_stream_f32), the phase multiplied by
                    the voicing and the equal-energy factor rsqrt(0.5 / phase) formed as the rows arrive
  _Noise            pushed, or drawn on the device up to the length the one-shot is certain to draw
  _BranchStage      a filter on one upstream track: PassThrough, the zero-phase FIR (the input samples and kernel rows of the
                    frames still to come: golf_ltv_fir_frames_fwd_f32 over a window that starts ceil(P/hop) frames early,
                    those frames dropped) or the frame-wise LPC filter (its last ceil(W/hop) - 1 filtered frames:
                    golf_lti_frames_ola_stream_f32, every frame filtered once, as soon as its samples and controls are there)
                    or an STFT-domain filter, LTVCepFilter / DiffWorldSPFilter (its last ceil(n_fft/hop) - 1 filtered frames,
                    its input from one sample before the next frame's start, the response rows of the frames still to come,
                    formed by the module's own code as the controls arrive: golf_stft_filter_frames_stream_f32)
  _AllPoleStage     the sample-wise all-pole end filter: the last M outputs (golf_ltv_allpole_fwd_state_f32)
  _Room             the LTI room filter: its last ``lead`` input samples (golf_lti_fir_f32 over an overlap window)
All of it is device memory; ``push`` reads nothing back from the device.  The bookkeeping is host integers derived from the
pushed lengths alone, composed from one set of primitives (source open / length / lookahead, branch open / final / lookahead).

Two wirings put the stages together, and four public classes check what they accept, parse ``push`` and pick a wiring:
  _Series     source + filtered noise -> end filter -> room filter.  ``DecoderStream`` (golf-ss: the all-pole end filter, whole
              LPC hops emitted) and ``FramewiseDecoderStream`` on golf-ff (a frame-wise branch on the running sum).
              Bookkeeping: ``emit_count`` / ``final_lengths`` / ``stream_latency`` over ``StreamGeometry``.
              ``SpectralDecoderStream`` (WORLD: a harmonic source, the STFT-domain end filter as a branch on the running
              sum).  Bookkeeping: ``spectral_emit_count`` / ``spectral_final_lengths`` / ``spectral_stream_latency`` over
              ``SpectralGeometry``.
  _Parallel   a branch on the source + a branch on the noise, summed over the shorter one -> room filter.
              ``HarmonicPlusNoiseStream`` (DDSP, the ISMIR'23 ddsp / sawsing / pulse / glottal_d vocoders, golf-v1, and NHV:
              the STFT-domain filter as the harmonic branch) and ``FramewiseDecoderStream`` on golf-v1.  Bookkeeping:
              ``hpn_emit_count`` / ``hpn_final_lengths`` / ``hpn_stream_latency`` over ``HPNGeometry``.
``open_stream`` returns whichever class fits a decoder: ``SpectralDecoderStream`` or ``HarmonicPlusNoiseStream`` for a decoder
with an STFT-domain filter (WORLD, NHV), else ``FramewiseDecoderStream`` or ``DecoderStream``; ``HarmonicPlusNoiseStream`` is
opened explicitly for the other harmonic-plus-noise decoders.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import cached_property
from typing import Optional, Tuple

import torch

from . import _lib
from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["BranchGeometry", "DecoderStream", "FramewiseDecoderStream", "HPNGeometry", "HarmonicPlusNoiseStream",
           "SpectralDecoderStream", "SpectralGeometry", "StreamGeometry", "emit_count", "final_lengths", "hpn_emit_count",
           "hpn_final_lengths", "hpn_stream_latency", "open_stream", "spectral_emit_count", "spectral_final_lengths",
           "spectral_stream_latency", "stream_latency"]


# ---- geometries ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BranchGeometry:
    """One filter stage on a track: a branch of a harmonic-plus-noise decoder, or a noise / end filter of a source-filter one."""
    kind: str = "pass"     # "pass" (PassThrough) | "fir" (LTVZeroPhaseFIRFilter) | "frames" (LTVMinimumPhaseFilter) | "stft"
    #                        (LTVCepFilter, DiffWorldSPFilter); within this module also "allpole": the sample-wise end filter
    hop: int = 1           # hop of its controls: the log magnitudes, gain / a, or the cepstra / mel envelope
    taps: int = 0          # fir: N = 2*(n_mag-1)
    window: int = 0        # frames: W; stft: n_fft
    centred: bool = True   # frames: False shifts the input by hop//2 and reflect-pads the output by as much

    @property
    def shift(self) -> int:   # hop//2 of centred=False
        return 0 if self.kind != "frames" or self.centred else self.hop // 2

    @property
    def reach(self) -> int:   # fir: R = N-1-(N-1)//2, the samples the zero-phase FIR reads after the one it writes
        return self.taps - 1 - (self.taps - 1) // 2 if self.taps else 0


@dataclass(frozen=True)
class StreamGeometry:
    """What the block bookkeeping of the source-filter streams depends on.  Hops are in output samples."""
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

    @cached_property
    def noise_branch(self) -> BranchGeometry:
        return BranchGeometry("fir", hop=self.fir_hop, taps=self.fir_taps) if self.fir_taps else BranchGeometry()

    @cached_property
    def lpc_branch(self) -> BranchGeometry:
        return BranchGeometry("frames", hop=self.hop, window=self.window) if self.window else \
            BranchGeometry("allpole", hop=self.hop)

    @property
    def fir_lookahead(self) -> int:
        return self.noise_branch.reach

    @property
    def parallel(self) -> bool:   # the frame-wise filter sits on the oscillator, not on the sum
        return bool(self.window) and self.hpn


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


@dataclass(frozen=True)
class SpectralGeometry:
    """What the bookkeeping of ``SpectralDecoderStream`` depends on: a harmonic source + filtered noise -> end filter."""
    phase_hop: int
    amp_hop: int = 0           # hop of the amplitude rows; 0: no amplitude track
    noise: BranchGeometry = field(default_factory=BranchGeometry)
    end: BranchGeometry = field(default_factory=BranchGeometry)
    source: str = "harmonic"

    @property
    def window(self) -> int:
        return self.end.window


# ---- bookkeeping primitives: sources -------------------------------------------------------------------------------------------
# The glottal source's functions take either geometry: they read ``phase_hop``, ``os``, ``half`` and ``w_hop`` alone.
def _glottal_len(g, n_phase: int) -> int:
    return GF.osc_lengths(n_phase, g.phase_hop, g.os)[1] if n_phase >= 1 else 0


def _glottal_open(g, n_phase: int, n_wsel: int) -> Tuple[int, int]:
    """(segments, samples) the glottal oscillator can render before the inputs end.  Coarse phase segment j reads p[j], p[j+1]
    and, for its fine samples m, table-select rows m // (w_hop*os) and the one after; decimated output o needs the fine samples
    o*os - half .. o*os + half."""
    if n_phase < 2 or n_wsel < 2:
        return 0, 0
    P = g.phase_hop * g.os
    nseg = max(0, min(n_phase - 1, ((n_wsel - 1) * g.w_hop * g.os) // P))
    fine = nseg * P
    return nseg, fine if g.os == 1 else max(0, (fine - 1 - g.half) // g.os + 1)


def _glottal_lookahead(g) -> int:
    """Input time past a sample of the glottal source by which it is determined: phase p[j+1] closes the decimator's last
    segment; the table-select row after the one a sample sits in."""
    return max(g.phase_hop + g.half // g.os, g.w_hop + (g.half + g.phase_hop * g.os - 1) // g.os, 1)


def _up_len(n: int, hop: int) -> int:
    return 0 if n < 1 else ((n - 1) * hop + 1 if hop > 1 else n)


def _source_open(g: HPNGeometry, n_phase: int, n_src: Optional[int]) -> Tuple[int, int]:
    """(segments, samples) of the source that can be rendered while the inputs are open: segment j needs p[j+1] and, for its
    last sample, the amplitude row after the one it sits in (glottal: ``_glottal_open``)."""
    if g.source == "glottal":
        return _glottal_open(g, n_phase, n_src)
    nseg = max(0, n_phase - 1)
    if g.amp_hop:
        nseg = min(nseg, max(0, (n_src - 1) * g.amp_hop) // g.phase_hop)
    return nseg, nseg * g.phase_hop


def _source_len(g: HPNGeometry, n_phase: int, n_src: Optional[int]) -> int:
    """The one-shot oscillator's length for these counts: final, and a lower bound while the inputs are open."""
    if g.source == "glottal":
        return _glottal_len(g, n_phase)
    n = _up_len(n_phase, g.phase_hop)
    return min(n, _up_len(n_src, g.amp_hop)) if g.amp_hop else n


def _noise_len(n_source: int, n_noise: Optional[int]) -> int:
    """Noise samples certain to exist: the one-shot draws (or truncates the given noise to) the oscillator's length, which is
    at least the length the phase pushed so far implies.  ``n_noise`` None: the noise is drawn on the device."""
    return n_source if n_noise is None else min(n_noise, n_source)


# ---- bookkeeping primitives: branches ------------------------------------------------------------------------------------------
def _branch_open(b: BranchGeometry, n_in: int, ctrl: Tuple[int, ...]) -> Tuple[int, int, int, int]:
    """(branch outputs finished, frames ready, filter outputs finished, filter inputs known) while the inputs are open, given
    ``n_in`` known input samples and the pushed control rows (fir: (log_mag,); frames, allpole: (gain, a)).
      fir      frame f reads its input up to (f+1)*hop - 1 + R
      frames   frame f reads x up to f*hop - pad + W - 1, a[f], and gain rows up to seg + 1 for the segment seg of its last
               sample, (f*hop - pad + W - 1) // hop = f + c; sample n is finished once its last frame, (n + pad) // hop, is
      allpole  whole LPC hops: frame E/hop must be there to close the last sample's frame
      stft     frame f reads x up to f*hop + pad - 1 (no reflection at the right edge while the input is open; frame 0 reads
               x[pad] through its left reflection) and response row f; sample n is finished once its last frame,
               (n + pad) // hop, is"""
    if b.kind == "pass":
        return n_in, 0, n_in, n_in
    if b.kind == "stft":
        pad = b.window // 2
        nfr = min(ctrl[0], (n_in - pad) // b.hop + 1) if n_in > pad else 0
        n_y = max(0, nfr * b.hop - pad)
        return n_y, nfr, n_y, n_in
    if b.kind == "fir":
        f = max(0, min(ctrl[0], (n_in - b.reach) // b.hop))
        return f * b.hop, f, f * b.hop, n_in
    if b.kind == "allpole":
        n = b.hop * max(0, min(n_in // b.hop, min(ctrl) - 1))
        return n, 0, n, n_in
    pad, n_x = b.window // 2, max(0, n_in - b.shift)
    c = (b.window - pad - 1) // b.hop
    nfr = max(0, min((n_x + pad - b.window) // b.hop + 1, ctrl[1], ctrl[0] - 1 - c))
    n_y = max(0, nfr * b.hop - pad)
    out = n_y if not b.shift else (n_y + b.shift if n_y > b.shift else 0)   # the reflect pad needs y[1 .. shift]
    return out, nfr, n_y, n_x


def _branch_final(b: BranchGeometry, n_in: int, ctrl: Tuple[int, ...],
                  short: str = "HarmonicPlusNoiseStream: {} samples are shorter than one FIR frame span") -> dict:
    """The one-shot filter's lengths for an input of ``n_in`` samples: its output (``out``) and, frame-wise, its input
    (``filter_in``, the one-shot's Tx after the shift), frames and filter output.  ``ctrl[0]``: its control frames."""
    if b.kind == "pass":
        return dict(out=n_in)
    if b.kind == "fir":
        span = n_in + 2 * ((b.taps - 1) // 2) - (b.taps + b.hop - 1)
        if span < 0:
            raise _lib.GolfError(short.format(n_in))
        return dict(out=min(span // b.hop + 1, ctrl[0]) * b.hop)
    F = ctrl[0]
    if b.kind == "stft":   # torch.stft(center=True, reflect) / istft: frames = min(1 + T // hop, F), hop * (frames - 1) samples
        nfr = min(1 + n_in // b.hop, F)
        if n_in <= b.window // 2 or nfr < 2:   # (the one-shot raises too: in torch.stft's reflect pad, or in torch.istft)
            raise _lib.GolfError(f"STFT-domain filter: {n_in} input samples with {F} control frames cannot be reflect-padded "
                                 f"by n_fft/2 = {b.window // 2} or make fewer than two frames")
        return dict(out=b.hop * (nfr - 1), filter_in=n_in, frames=nfr)
    if b.kind == "allpole":
        return dict(out=GF.ss_output_length(n_in, F, b.hop) if F >= 1 and n_in >= 1 else 0)
    x = n_in - b.shift
    Tx, nfr, Ty = GF.ff_output_length(x, F, b.hop, b.window) if x >= 1 and F >= 2 else (0, 0, 0)
    if nfr > F:
        raise _lib.GolfError(f"frame-wise filter: {nfr} frames needed but only {F} coefficient frames")
    if b.shift and Ty <= b.shift:
        raise _lib.GolfError(f"frame-wise filter (centred=False): {Ty} output samples cannot be reflect-padded by {b.shift}")
    return dict(out=Ty + b.shift, filter_in=Tx, frames=nfr, filter_out=Ty)


def _branch_lookahead(b: BranchGeometry, L_in: int) -> int:
    """Input time past an output sample of the branch by which it is determined, ``L_in`` being that of its input."""
    if b.kind == "pass":
        return L_in
    if b.kind == "fir":
        return b.hop - 1 + b.reach + L_in
    if b.kind == "allpole":
        return b.hop - 1 + L_in   # the emission granularity (whole LPC frames)
    if b.kind == "stft":          # sample t waits for frame (t + pad) // hop, whose samples reach t + n_fft - 1
        return b.window - 1 + L_in
    pad, s = b.window // 2, b.shift
    c = (b.window - pad - 1) // b.hop
    q = max(b.window - 1 + L_in, pad - s + b.hop * (c + 1))
    if s:   # centred=False: outputs 0 .. s-1 wait for output 2s, whose frame f0 reads input up to f0*hop - pad + W - 1 + s
        f0 = (s + pad) // b.hop
        q = max(q, f0 * b.hop - pad + b.window - 1 + s + L_in, b.hop * (f0 + c + 1))
    return q


# ---- the public bookkeeping ----------------------------------------------------------------------------------------------------
def _series_open(g: StreamGeometry, n_phase: int, n_wsel: int, n_noise: Optional[int], n_logmag: int, n_gain: int,
                 n_a: int) -> Tuple[int, int, int, int, int]:
    """(oscillator segments, its samples, noise samples, filtered noise samples, E) while the utterance is open."""
    nseg, n_osc = _glottal_open(g, n_phase, n_wsel)
    n_nz_in = _noise_len(_glottal_len(g, n_phase), n_noise)
    n_nz = _branch_open(g.noise_branch, n_nz_in, (n_logmag,))[0]
    if g.parallel:
        return nseg, n_osc, n_nz_in, n_nz, min(_branch_open(g.lpc_branch, n_osc, (n_gain, n_a))[0], n_nz)
    return nseg, n_osc, n_nz_in, n_nz, _branch_open(g.lpc_branch, min(n_osc, n_nz), (n_gain, n_a))[0]


def emit_count(g: StreamGeometry, n_phase: int, n_wsel: int, n_noise: Optional[int], n_logmag: int, n_gain: int,
               n_a: int) -> int:
    """E: the output samples [0, E) a stream emits once these many steps of each track have been pushed (``n_noise`` None: the
    noise is drawn on the device).  Every sample below it is determined -- through the operators' stencils -- by what has been
    pushed: osc (phase + table select, decimator context), filtered noise, and the gain / a frames of the LPC filter
    (``_branch_open``: whole LPC hops with the sample-wise end filter; with the frame-wise filter every sample whose frames
    are all ready)."""
    return _series_open(g, n_phase, n_wsel, n_noise, n_logmag, n_gain, n_a)[4]


def final_lengths(g: StreamGeometry, n_phase: int, n_noise: Optional[int], n_logmag: int, n_frames: int) -> dict:
    """Lengths of the one-shot decoder's stages once the inputs have ended (``n_frames``: gain / a frames).  With the
    frame-wise filter also its input length (``filter_in``, the one-shot's Tx), frames (``frames``) and output length
    (``filter_out``); golf-v1's output is the shorter of the filtered oscillator and the filtered noise."""
    osc = _glottal_len(g, n_phase)
    noise = _noise_len(osc, n_noise)
    nz = _branch_final(g.noise_branch, noise, (n_logmag,),
                       "DecoderStream: {} noise samples are shorter than one noise-filter frame span")["out"]
    src = osc if g.parallel else min(osc, nz)
    f = _branch_final(g.lpc_branch, src, (n_frames, n_frames))
    if not g.window:
        return dict(osc=osc, noise=noise, noise_filter=nz, source=src, out=f["out"])
    return dict(osc=osc, noise=noise, noise_filter=nz, source=src, filter_in=f["filter_in"], frames=f["frames"],
                filter_out=f["filter_out"], out=min(f["out"], nz) if g.hpn else f["out"])


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
    L_osc = _glottal_lookahead(g)
    L_nz = _branch_lookahead(g.noise_branch, g.phase_hop - 1)
    if g.parallel:
        return max(_branch_lookahead(g.lpc_branch, L_osc), L_nz)
    return _branch_lookahead(g.lpc_branch, max(L_osc, L_nz))


def hpn_emit_count(g: HPNGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int], harm_ctrl: Tuple[int, ...],
                   noise_ctrl: Tuple[int, ...]) -> int:
    """E: the output samples [0, E) ``HarmonicPlusNoiseStream`` emits once these many steps of each track have been pushed.
    ``n_phase``: phase steps (with voicing, the steps both tracks have); ``n_src``: amplitude rows (harmonic source; None
    without an amplitude track) or table-select rows (glottal); ``n_noise`` None: the noise is drawn on the device;
    ``harm_ctrl`` / ``noise_ctrl``: each branch's control rows, () / (log_mag,) / (gain, a).  Every sample below E is
    determined by what has been pushed: the source's segments, the noise the one-shot is certain to draw, and each branch's
    stencil; the output is the sum of the two branches over the shorter one."""
    n_osc = _source_open(g, n_phase, n_src)[1]
    nz = _noise_len(_source_len(g, n_phase, n_src), n_noise)
    return min(_branch_open(g.harm, n_osc, harm_ctrl)[0], _branch_open(g.noise, nz, noise_ctrl)[0])


def hpn_final_lengths(g: HPNGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int], harm_ctrl: Tuple[int, ...],
                      noise_ctrl: Tuple[int, ...]) -> dict:
    """Lengths of the one-shot decoder's stages once the inputs have ended: the oscillator (``source``), the noise, each
    branch (``harm``, ``noise_branch``: dicts of ``_branch_final``) and the output, the shorter branch."""
    src = _source_len(g, n_phase, n_src)
    noise = _noise_len(src, n_noise)
    h = _branch_final(g.harm, src, harm_ctrl)
    n = _branch_final(g.noise, noise, noise_ctrl)
    return dict(source=src, noise=noise, harm=h, noise_branch=n, out=min(h["out"], n["out"]))


def hpn_stream_latency(g: HPNGeometry) -> int:
    """Worst-case lookahead of ``HarmonicPlusNoiseStream`` in samples: output sample t is emitted at the latest once every
    track has been pushed up to input time t + latency.  Per stage, the input time past a sample that determines it:
      harmonic source   P + A - gcd(P, A)  (P the phase hop, A the amplitude hop: p[j+1] closes segment j, the segment's last
                        sample needs the amplitude row after its own; P without amplitudes)
      glottal source    as ``stream_latency`` (phase, table select, decimator)
      noise             max(P - 1, A - 1): the samples the one-shot is certain to draw
      FIR branch        + fir_hop - 1 + R  (R = N-1-(N-1)//2 samples read past the one written)
      frame-wise branch max(W - 1 + input, pad - s + hop * ((W - pad - 1) // hop + 1)) + 2 s   (s = hop//2 without centring)
      STFT branch       + n_fft - 1  (the last frame that covers a sample reaches n_fft - 1 samples past it)
    and the output waits for both branches.  DDSP (phase at hop 1, amplitudes at 240, FIR 510 at 240): 239 + 239 + 255 = 733.  NHV (phase
    at hop 1, n_fft 1024 on the pulse train, FIR 510 at 240): max(1023 + 1, 239 + 255) = 1024."""
    L_src, L_nz = _source_lookahead(g)
    return max(_branch_lookahead(g.harm, L_src), _branch_lookahead(g.noise, L_nz))


def _source_lookahead(g) -> Tuple[int, int]:
    """(source, noise): the input time past a sample of the source, and of the noise the one-shot is certain to draw, by
    which it is determined (``hpn_stream_latency``).  ``g``: HPNGeometry or SpectralGeometry."""
    P = g.phase_hop
    if g.source == "glottal" and g.os > 1:
        return _glottal_lookahead(g), P - 1
    # (a glottal source without a decimator: the table-select rows as amplitudes; ``stream_latency`` keeps the looser
    #  ``_glottal_lookahead`` there)
    A = g.w_hop if g.source == "glottal" else g.amp_hop
    return P + A - math.gcd(P, A) if A else P, P - 1 if g.source == "glottal" else max(P - 1, A - 1 if A else 0)


def _spectral_open(g: SpectralGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int],
                   noise_ctrl: Tuple[int, ...], end_ctrl: Tuple[int, ...]) -> Tuple[int, int, int, int, int]:
    """(oscillator segments, its samples, noise samples, filtered noise samples, E) while the utterance is open."""
    nseg, n_osc = _source_open(g, n_phase, n_src)
    n_nz_in = _noise_len(_source_len(g, n_phase, n_src), n_noise)
    n_nz = _branch_open(g.noise, n_nz_in, noise_ctrl)[0]
    return nseg, n_osc, n_nz_in, n_nz, _branch_open(g.end, min(n_osc, n_nz), end_ctrl)[0]


def spectral_emit_count(g: SpectralGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int],
                        noise_ctrl: Tuple[int, ...], end_ctrl: Tuple[int, ...]) -> int:
    """E: the output samples [0, E) ``SpectralDecoderStream`` emits once these many steps of each track have been pushed
    (arguments as ``hpn_emit_count``; ``end_ctrl``: the end filter's control rows).  The end filter runs on the sum of the
    source and the filtered noise as far as both are known; a sample is out once every STFT frame that covers it is ready."""
    return _spectral_open(g, n_phase, n_src, n_noise, noise_ctrl, end_ctrl)[4]


def spectral_final_lengths(g: SpectralGeometry, n_phase: int, n_src: Optional[int], n_noise: Optional[int],
                           noise_ctrl: Tuple[int, ...], end_ctrl: Tuple[int, ...]) -> dict:
    """Lengths of the one-shot decoder's stages once the inputs have ended: oscillator, noise, filtered noise, their sum
    (``source`` = ``filter_in``), the end filter's frames and the output."""
    osc = _source_len(g, n_phase, n_src)
    noise = _noise_len(osc, n_noise)
    nz = _branch_final(g.noise, noise, noise_ctrl,
                       "SpectralDecoderStream: {} noise samples are shorter than one noise-filter frame span")["out"]
    src = min(osc, nz)
    return dict(osc=osc, noise=noise, noise_filter=nz, source=src, **_branch_final(g.end, src, end_ctrl))


def spectral_stream_latency(g: SpectralGeometry) -> int:
    """Worst-case lookahead of ``SpectralDecoderStream`` in samples, composed as ``hpn_stream_latency`` composes it: the end
    filter's n_fft - 1 on top of the later of the source and the filtered noise.  WORLD (n_fft 1024, phase at hop 1, FIR 510
    at hop 240): 1023 + max(1, 239 + 255) = 1517."""
    L_src, L_nz = _source_lookahead(g)
    return _branch_lookahead(g.end, max(L_src, _branch_lookahead(g.noise, L_nz)))


# ---- tracks --------------------------------------------------------------------------------------------------------------------
class _Track:
    """A device buffer of one input or intermediate track along dim 1, holding global steps [start, start + n)."""

    def __init__(self, start: int = 0, data: torch.Tensor = None):
        self.start = start
        self.data = data

    @property
    def end(self) -> int:
        return self.start + (0 if self.data is None else self.data.shape[1])

    def append(self, x: torch.Tensor, fresh: bool = False) -> None:
        """``fresh``: x is a stage's own result, which nobody else writes -- it becomes the buffer of an emptied track as it
        is (no copy)."""
        if x.shape[1] == 0 and self.data is not None:
            return
        if self.data is None or (fresh and self.data.shape[1] == 0):
            self.data = x
        else:
            self.data = torch.cat([self.data, x], 1)

    def get(self, lo: int, hi: int) -> torch.Tensor:
        assert self.start <= lo <= hi <= self.end, (self.start, lo, hi, self.end)
        return self.data[:, lo - self.start: hi - self.start]

    def drop_before(self, lo: int) -> None:
        lo = min(max(lo, self.start), self.end)
        if lo > self.start:
            self.data = self.data[:, lo - self.start:]
            self.start = lo


def _take_sum(a: _Track, b: _Track, lo: int, hi: int) -> torch.Tensor:
    """a[lo:hi] + b[lo:hi], both tracks trimmed to ``hi``: the one consumer of both has read them."""
    y = a.get(lo, hi) + b.get(lo, hi)
    a.drop_before(hi)
    b.drop_before(hi)
    return y


def _check_lpc_tracks(g: _Track, a: _Track, who: str) -> None:
    if g.end != a.end:
        raise ValueError(f"{who}.finish: {g.end} gain frames but {a.end} coefficient frames")


def _f32(t: AudioTensor, dev) -> torch.Tensor:
    # (autocast: fp16 / bf16 control tracks become fp32 here, before any kernel sees them)
    return t.as_tensor().to(device=dev, dtype=torch.float32)


# ---- stages --------------------------------------------------------------------------------------------------------------------
class _Source:
    """What the two oscillators share: the phase the oscillator sees (phase * voicing, as HarmonicPlusNoiseSynth.forward forms
    it), the next segment to render and the exact Q0.64 phase before it.  ``out``: the oscillator's samples."""

    def __init__(self, B: int, dev, voiced: bool):
        self.B, self._dev, self.voiced = B, dev, voiced
        self.praw, self.vraw, self.ph, self.out = _Track(), _Track(), _Track(), _Track()
        self.seg = 0
        self.acc = torch.zeros(B, dtype=torch.int64, device=dev)

    @property
    def n_phase_pushed(self) -> int:
        return self.praw.end if self.voiced else self.ph.end

    def check(self, params, who: str) -> None:   # what a source refuses in a later push, and at finish
        pass

    def check_final(self, who: str) -> None:
        pass

    def append_phase(self, phase: AudioTensor, voicing: Optional[AudioTensor]) -> torch.Tensor:
        """Returns the new steps of the oscillator's phase."""
        p = _f32(phase, self._dev)
        if not self.voiced:
            self.ph.append(p)
            return p
        self.praw.append(p)
        self.vraw.append(_f32(voicing, self._dev))
        lo, n = self.ph.end, min(self.praw.end, self.vraw.end)
        p = self.praw.get(lo, n) * self.vraw.get(lo, n)
        self.ph.append(p)
        self.praw.drop_before(n)
        self.vraw.drop_before(n)
        return p


class _GlottalSource(_Source):
    """The indexed glottal table from a carried phase, and its decimator over the fine samples kept for it.  ``g``: either
    geometry (``phase_hop``, ``os``, ``half``, ``w_hop``)."""
    rows_name = "table select"

    @staticmethod
    def decimator(osc) -> dict:
        """The geometry fields the oscillator module fixes."""
        os_ = int(osc.oversampling)
        return dict(os=os_, half=(osc.decimater.taps.numel() - 1) // 2 if os_ > 1 else 0)

    def __init__(self, osc, g, B: int, dev, voiced: bool = False):
        super().__init__(B, dev, voiced)
        self.g = g
        self.rows_hop = g.w_hop
        self._taps = osc.decimater.taps.float().contiguous() if g.os > 1 else None
        self._table = osc.table.detach().float().contiguous()
        self._equal_energy = osc.equal_energy
        self.w = _Track()
        pad = -(-g.half // g.os) * g.os   # zeros before fine sample 0: the one-shot decimator's own zero padding
        self._pre = _Track(-pad, torch.zeros(B, pad, device=dev))

    def rows(self) -> int:
        return self.w.end

    def append(self, phase, voicing, params) -> None:
        self.append_phase(phase, voicing)
        self.w.append(_f32(params[0], self._dev))

    def check_final(self, who: str) -> None:
        if self.ph.end >= 1 and self.w.end < 1:
            raise ValueError(f"{who}.finish: no table-select frame was pushed")

    def run(self, nseg: int, n_osc: int, final: bool) -> None:
        """Render the segments below ``nseg`` (at finish: all of them and the one-shot's last point) and decimate up to
        ``n_osc`` output samples."""
        g, P = self.g, self.g.phase_hop * self.g.os
        n_phase = self.ph.end
        if final:
            nseg = n_phase - 1 if n_phase >= 1 else 0
        last = final and n_phase >= 1
        if nseg > self.seg or last:
            j0 = self.seg
            ph = self.ph.get(j0, min(nseg + 1, n_phase))
            r_lo = min((j0 * P) // (g.w_hop * g.os), self.w.end - 1)   # (past the last row: the kernel repeats it)
            wsel = self.w.get(r_lo, self.w.end)
            pre = GF.glottal_osc_stream(ph, j0, nseg - j0, last, g.phase_hop, g.os, wsel, r_lo, g.w_hop, self._table,
                                        self._equal_energy, self.acc)
            self._pre.append(pre)
            self.seg = nseg
            self.ph.drop_before(nseg)   # p[nseg] closes the next segment
            self.w.drop_before(min((nseg * P) // (g.w_hop * g.os), self.w.end - 1))
        if n_osc <= self.out.end:
            return
        if g.os == 1:
            self.out.append(self._pre.get(self.out.end, n_osc))
            self._pre.drop_before(n_osc)
            return
        o_base = self._pre.start // g.os
        y = GF.decimate_fir(self._pre.data, self._taps, g.os)
        self.out.append(y[:, self.out.end - o_base: n_osc - o_base])
        self._pre.drop_before(((n_osc * g.os - g.half) // g.os) * g.os)


class _HarmonicSource(_Source):
    """The harmonic oscillator bank (HarmonicOscillator, AdditiveSynthesizer, V1AdditiveSynthesizer, SawToothOscillator,
    AdditivePulseTrain) from a carried phase.  ``amp_hop``: hop of the amplitude rows, 0 without an amplitude track."""
    rows_name = "amplitudes"

    @staticmethod
    def takes_amplitudes(osc) -> bool:
        from .synth import AdditivePulseTrain, SawToothOscillator

        return type(osc) not in (SawToothOscillator, AdditivePulseTrain)

    def __init__(self, osc, P: int, params, B: int, dev, voiced: bool, refuse):
        from .synth import AdditivePulseTrain, AdditiveSynthesizer, SawToothOscillator

        super().__init__(B, dev, voiced)
        self.P, self.amp_hop, self._ts_mode = P, 0, None
        if self.takes_amplitudes(osc):
            A = self.amp_hop = int(params[0].hop_length)
            if type(osc) is AdditiveSynthesizer and P != 1:
                if A != P:
                    refuse(f"AdditiveSynthesizer with the phase at hop {P} and the amplitudes at hop {A} (the phase "
                           "hop must be 1 or the amplitude hop)")
                self._ts_mode = "fold"
            elif type(osc) is AdditiveSynthesizer:
                self._ts_mode = "phase"
            if P > 1 and A % P:
                refuse(f"amplitudes at hop {A} with the phase at hop {P} (a multiple of the phase hop is needed)")
            self.H = int(params[0].shape[2])
        elif type(osc) is SawToothOscillator:
            self.H = int(osc.amplitudes.numel())
        else:
            self.H = int(osc.num_harmonics)
        if type(osc) is AdditivePulseTrain:
            self._ts_mode = "phase"
        self._hscale = osc.amplitudes.detach().float().to(dev).contiguous() if type(osc) is SawToothOscillator else None
        self.rows_hop = self.amp_hop
        self._amp, self._araw, self._sc = _Track(), _Track(), _Track()

    def rows(self) -> Optional[int]:
        return self._amp.end if self.amp_hop else None

    def check(self, params, who: str) -> None:
        if self.amp_hop and int(params[0].shape[2]) != self.H:
            raise ValueError(f"{who}.push: the number of harmonics changed between pushes")

    def append(self, phase, voicing, params) -> None:
        p = self.append_phase(phase, voicing)
        if self._ts_mode is not None and p.shape[1]:   # rsqrt(0.5 / phase): the equal-energy factor (synth.py _sqrt_two_phase)
            self._sc.append(torch.rsqrt(0.5 / p))
        if not self.amp_hop:
            return
        if self._ts_mode != "fold":
            self._amp.append(_f32(params[0], self._dev))
            return
        self._araw.append(_f32(params[0], self._dev))   # amplitudes * unsqueeze(scale, -1), row by row as both arrive
        lo, m = self._amp.end, min(self._araw.end, self._sc.end)
        if m > lo:
            self._amp.append(self._araw.get(lo, m) * torch.unsqueeze(self._sc.get(lo, m), -1))
            self._araw.drop_before(m)
            self._sc.drop_before(m)

    def run(self, nseg: int, n_osc: int, final: bool) -> None:
        """Render segments [self.seg, nseg) (+ at finish the sample k = 0 of segment nseg: the one-shot's last sample)."""
        P, A = self.P, self.amp_hop
        if final:
            nseg = (n_osc - 1) // P if n_osc else 0
        last = final and n_osc >= 1
        if nseg <= self.seg and not last:
            return
        j0 = self.seg
        n = (nseg - j0) * P + int(last)
        t_lo, t_hi = j0 * P, j0 * P + n - 1
        kw = {}
        if A:
            end = self._amp.end if last else -1
            row = lambda t: min(t // A, end - 2) if end >= 2 else (0 if end == 1 else t // A)
            r_lo, r_hi = row(t_lo), min(self._amp.end, row(t_hi) + 2)
            kw.update(amp=self._amp.get(r_lo, r_hi), a_first=r_lo, a_end=end, amp_hop=A)
        if self._ts_mode == "phase":   # tscale rows are the phase rows
            kw.update(tscale=self._sc.get(self._sc.start, self._sc.end), s_first=self._sc.start,
                      s_end=self._sc.end if last else -1, ts_hop=P)
        y = GF.harmonic_osc_stream(self.ph.get(j0, nseg + 1), j0, nseg - j0, last, P, self.H, self.acc,
                                   hscale=self._hscale, **kw)
        self.out.append(y)
        self.seg = nseg
        self.ph.drop_before(nseg)        # p[nseg] closes the next segment
        # rows the next call reads: from the next sample's row on, and the last two (the end clamp interpolates between them)
        if A:
            self._amp.drop_before(min((nseg * P) // A, self._amp.end - 2))
        if self._ts_mode == "phase":
            self._sc.drop_before(min(nseg, self._sc.end - 2))


class _Noise:
    """The noise track ``out``: pushed with every block, or drawn as StandardNormalNoise draws it."""

    def __init__(self, B: int, dev, pushed: bool, generated: bool):
        self.B, self._dev, self.generated = B, dev, generated
        self.out = _Track()
        self.pushed = 0 if pushed else None   # samples pushed; None: drawn on the device

    def check(self, noise, who: str) -> None:
        if (noise is None) != (self.pushed is None):
            raise ValueError(f"{who}.push: pass noise= in every push or in none")

    def append(self, noise: Optional[AudioTensor]) -> None:
        if noise is not None:
            x = _f32(noise, self._dev)
            self.out.append(x)
            self.pushed += x.shape[1]

    def run(self, n: int) -> None:
        if self.generated and n > self.out.end:
            self.out.append(torch.randn(self.B, n - self.out.end, device=self._dev))


class _BranchStage:
    """One filter run block by block.  It reads its input from the upstream track ``src`` (which it alone consumes and trims)
    and appends its finished output samples to ``out`` (global indices; PassThrough: ``out`` is ``src``)."""

    def __init__(self, b: BranchGeometry, module, src: _Track, B: int, dev):
        self.b, self.src, self.B, self._dev = b, src, B, dev
        self.out = src if b.kind == "pass" else _Track()
        self.n_ctrl = 0
        self._frames = 0
        if b.kind == "fir":
            self._kern = _Track()
            self._window = module._window(b.taps, dev)
            self._basis = GF.zero_phase_fir_basis(b.taps // 2 + 1, dev)
        elif b.kind == "frames":
            self._g, self._a, self._y = _Track(), _Track(), _Track()
            self._win = module._window.detach().float().to(dev).contiguous()
            self._filtered = self._n_x = 0
            self._carry = None
        elif b.kind == "stft":
            self._module = module
            self._H = _Track()
            self._win = module._window.detach().float().to(dev).contiguous()
            self._filtered = 0
            self._carry = None
            self._width = None

    @staticmethod
    def geometry(kind: str, module, params, who: str, role: str = "") -> BranchGeometry:
        """The branch's geometry from the tracks of the first push."""
        if kind == "fir":
            return BranchGeometry("fir", hop=int(params[0].hop_length), taps=2 * (int(params[0].shape[2]) - 1))
        if kind == "frames":
            if int(params[0].hop_length) != int(params[1].hop_length):
                raise ValueError(f"{who}: {role}gain at hop {params[0].hop_length}, a at hop {params[1].hop_length}")
            hop, W = int(params[1].hop_length), int(module._window.numel())
            if W < 2 * hop:
                raise ValueError(f"{who}: {role}window {W} < 2*hop {2 * hop}")
            return BranchGeometry("frames", hop=hop, window=W, centred=bool(module.centred))
        if kind == "stft":
            if int(params[0].hop_length) != int(module.hop_length):
                raise ValueError(f"{who}: {role}controls at hop {params[0].hop_length}, the filter's hop is {module.hop_length}")
            return BranchGeometry("stft", hop=int(module.hop_length), window=int(module.n_fft))
        return BranchGeometry()

    def ctrl(self) -> Tuple[int, ...]:
        """The control rows pushed so far: () / (log_mag,) / (gain, a)."""
        if self.b.kind in ("fir", "stft"):
            return (self.n_ctrl,)
        return (self._g.end, self._a.end) if self.b.kind == "frames" else ()

    def check(self, params, who: str) -> None:
        if self.b.kind == "fir" and 2 * (int(params[0].shape[2]) - 1) != self.b.taps:
            raise ValueError(f"{who}.push: the FIR bins changed between pushes")
        if self.b.kind == "frames" and self._a.data is not None and params[1].shape[2] != self._a.data.shape[2]:
            raise ValueError(f"{who}.push: the LPC order changed between pushes")
        if self.b.kind == "stft" and self._width not in (None, int(params[0].shape[2])):
            raise ValueError(f"{who}.push: the width of the STFT-domain filter's controls changed between pushes")

    def _response(self, ctrl: torch.Tensor) -> torch.Tensor:
        """(B, rows, n_fft/2 + 1) response rows from control rows, by the module's own code: the rows of the one-shot's H."""
        return self._module.response_rows(ctrl)

    def append(self, params) -> None:
        if self.b.kind == "stft":
            c = params[0]
            self._width = int(c.shape[2])
            if c.shape[1]:
                self._H.append(self._response(_f32(c, self._dev)))
            self.n_ctrl += c.shape[1]
            return
        if self.b.kind == "fir":
            lm = params[0]
            if lm.shape[1]:
                x = _f32(lm, self._dev).contiguous()
                kern = GF._fir_kernels_raw(GF.ZERO_PHASE_FIR, x, self._window, self._basis)
                self._kern.append(kern.view(self.B, x.shape[1], -1))
            self.n_ctrl += lm.shape[1]
        elif self.b.kind == "frames":
            self._g.append(_f32(params[0], self._dev))
            self._a.append(_f32(params[1], self._dev).contiguous())

    def check_final(self, who: str) -> None:
        if self.b.kind == "frames":
            _check_lpc_tracks(self._g, self._a, who)

    def run(self, n_in: int, final: bool, fin: Optional[dict], who: str = "") -> None:
        """The input is known up to ``n_in`` samples (at finish: the one-shot's input length, ``fin`` its lengths)."""
        if self.b.kind == "fir":
            self._run_fir(n_in, final, fin)
        elif self.b.kind == "frames":
            if final:
                self.check_final(who)
            self._run_frames(n_in, final, fin)
        elif self.b.kind == "stft":
            self._run_stft(n_in, final, fin)

    def _run_stft(self, n_in: int, final: bool, fin) -> None:
        """Filter the STFT frames that are ready and write the samples they finish (golf_stft_filter_frames_stream_f32)."""
        b = self.b
        if final:
            n_y, nfr = fin["out"], fin["frames"]
        else:
            n_y, nfr = _branch_open(b, n_in, self.ctrl())[:2]
        f0, n0 = self._frames, self._filtered
        if nfr <= f0 and n_y <= n0:
            return
        y, self._carry = GF.stft_filter_stream(
            self.src.get(self.src.start, self.src.end), self._H.data, self._win, b.hop, self._carry, x0=self.src.start,
            h0=self._H.start, f0=f0, nf=max(0, nfr - f0), n0=n0, ny=max(0, n_y - n0), x_end=n_in if final else -1,
            frames_end=nfr if final else -1)
        self._frames, self._filtered = max(f0, nfr), max(n0, n_y)
        # the next frame starts at frames*hop - pad; should it turn out to be the utterance's last, of a length that is a
        # multiple of hop, its right reflection reads one sample before that
        self.src.drop_before(max(0, self._frames * b.hop - b.window // 2 - 1))
        self._H.drop_before(self._frames)
        self.out.append(y, fresh=True)

    def _run_fir(self, n_in: int, final: bool, fin) -> None:
        b = self.b
        f_lo = self._frames
        f_hi = fin["out"] // b.hop if final else _branch_open(b, n_in, self.ctrl())[1]
        if f_hi <= f_lo:
            return
        q = -(-((b.taps - 1) // 2) // b.hop)          # frames whose left context would be the call's zero padding
        fs = max(0, f_lo - q)
        e = n_in if final else min(n_in, f_hi * b.hop + b.reach)
        x = self.src.get(fs * b.hop, e)
        kern = self._kern.data
        Fk = kern.shape[1]
        y = GF._FIRFrames.apply(x, kern.reshape(self.B * Fk, -1), Fk, b.taps, b.hop, fs - self._kern.start, False)
        self.out.append(y[:, (f_lo - fs) * b.hop: (f_hi - fs) * b.hop], fresh=True)
        self._frames = f_hi
        nxt = max(0, f_hi - q)
        self.src.drop_before(nxt * b.hop)
        self._kern.drop_before(nxt)

    def _run_frames(self, n_in: int, final: bool, fin) -> None:
        """Filter the frames that are ready and write the samples they finish.  The filter's input x is ``src`` from sample
        ``shift`` on: x[n] = src[n + shift]."""
        b, s = self.b, self.b.shift
        if final:
            n_x, nfr, n_y = fin.get("filter_in", 0), fin.get("frames", 0), fin.get("filter_out", 0)
            n_out = fin["out"]
        else:
            n_out, nfr, n_y, n_x = _branch_open(b, n_in, self.ctrl())
        self._n_x = max(self._n_x, n_x)   # (x once known stays part of the window, also past the utterance's final Tx)
        f0, n0 = self._frames, self._filtered
        if nfr > f0 or n_y > n0:
            # (a frame or a sample to write implies n_x >= 1, and every track holds a tensor from the first push on)
            self.src.drop_before(s)
            y, self._carry = GF.lti_frames_ola_stream(
                self.src.get(self.src.start, self._n_x + s), self._g.data, self._a.data, self._win, b.hop, self._carry,
                x0=self.src.start - s, g0=self._g.start, a0=self._a.start, f0=f0, nf=max(0, nfr - f0), n0=n0,
                ny=max(0, n_y - n0), x_end=n_x if final else -1, g_end=self._g.end if final else -1)
            self._frames, self._filtered = max(f0, nfr), max(n0, n_y)
            t_next = max(0, self._frames * b.hop - b.window // 2)   # the first sample the next frame reads
            self.src.drop_before(t_next + s)
            self._g.drop_before(t_next // b.hop)
            self._a.drop_before(self._frames)
            if not s:
                self.out.append(y, fresh=True)
                return
            self._y.append(y)
        if s and n_out > self.out.end:
            if self.out.end == 0:   # the one-shot's reflect pad: outputs 0 .. s-1 are filter outputs s .. 1
                self.out.append(self._y.get(1, s + 1).flip(1))
            self.out.append(self._y.get(self.out.end - s, n_out - s))
            self._y.drop_before(n_out - s)


class _AllPoleStage:
    """The sample-wise all-pole end filter of golf-ss: y[<0] = 0, the last M outputs carried.  The last block is kept for the
    utterance's final sample."""

    def __init__(self, hop: int, M: int, B: int, dev):
        self.hop, self.M, self._dev = hop, M, dev
        self._g, self._a = _Track(), _Track()
        self._state = torch.zeros(B, M, device=dev)
        self._last_block = None

    def ctrl(self) -> Tuple[int, int]:
        return (self._g.end, self._a.end)

    def check(self, params, who: str) -> None:
        if params[1].shape[2] != self.M:
            raise ValueError(f"{who}.push: the LPC order changed between pushes")

    def append(self, params) -> None:
        self._g.append(_f32(params[0], self._dev))
        self._a.append(_f32(params[1], self._dev).contiguous())

    def check_final(self, who: str) -> None:
        _check_lpc_tracks(self._g, self._a, who)

    def run(self, src: torch.Tensor, lo: int, E: int, final: bool) -> torch.Tensor:
        """Filter ``src``, the source samples [lo, E)."""
        hop = self.hop
        f0 = lo // hop
        f1 = min(self._g.end - 1, (E - 1) // hop + 1)
        if final and f1 == f0 and self._last_block is not None:
            # the utterance's last sample alone in its frame: its interpolation runs between the last two frames, which only
            # the block before spans -- run that block again from its saved state, one sample longer, and keep that sample
            state, src0, b_lo = self._last_block
            f0 = b_lo // hop
            x, st, skip = torch.cat([src0, src], 1), state.clone(), src0.shape[1]
        else:
            self._last_block = (self._state.clone(), src, lo)
            x, st, skip = src, self._state, 0
        y = GF.ltv_allpole_ss_state(x, self._g.get(f0, f1 + 1), self._a.get(f0, f1 + 1), hop, st)
        if not skip:
            self._g.drop_before(f0)   # (the frames of this block stay for _last_block)
            self._a.drop_before(f0)
        return y[:, skip:]


class _Room:
    """The LTI room filter over the carried ``lead`` samples before the block (zeros before sample 0)."""

    def __init__(self, room, B: int, dev):
        self.lead = room._padding
        self.taps = torch.cat([room.kernel.detach(), room._tail.to(room.kernel.dtype)]).float().contiguous()
        self.hist = torch.zeros(B, self.lead, device=dev)

    def run(self, y: torch.Tensor) -> torch.Tensor:
        x = torch.cat([self.hist, y], 1)
        self.hist = x[:, x.shape[1] - self.lead:]
        return GF.lti_fir(x, self.taps, self.lead)[:, self.lead:]


# ---- wirings -------------------------------------------------------------------------------------------------------------------
def _require_device(t, who: str) -> None:
    if t.device.type != "cuda":
        raise _lib.GolfError(f"{who}: golf_amd kernels need ROCm device tensors; there is no CPU path")


def _check_tracks(want, B: int, who: str) -> None:
    for t, hop, name in want:
        if int(t.hop_length) != hop or t.shape[0] != B:
            raise ValueError(f"{who}.push: {name} of shape {tuple(t.shape)} at hop {t.hop_length}; the stream has B={B}, "
                             f"hop {hop}")


class _Series:
    """source + filtered noise -> end filter -> room filter: golf-ss (``lpc`` None: the sample-wise all-pole filter), golf-ff
    (``lpc``: the frame-wise filter module) and, on a harmonic source, WORLD (``lpc``: the STFT-domain filter module).  Built
    from the tracks of the first push; every push after it passes ``check``, ``append`` and ``advance`` with the same
    arguments ``(phase, osc_params, end_params, lm, noise)`` -- ``osc_params`` (wsel,) for the glottal table, ``end_params``
    (gain, a) or the STFT-domain filter's (controls,), ``lm`` None without a noise filter.  ``checks_first``: at finish, the
    tracks' own faults are reported before those of the lengths.  The glottal source keeps its books with ``StreamGeometry``
    (``_series_open`` / ``final_lengths``), the harmonic one with ``SpectralGeometry``."""

    def __init__(self, who: str, decoder, lpc, B: int, generated_noise: bool, checks_first: bool, phase, osc_params,
                 end_params, lm, noise, refuse=None):
        dev = phase.device
        _require_device(phase, who)
        osc = decoder.harm_oscillator
        b_lpc = _BranchStage.geometry(_branch_kind(lpc), lpc, end_params, who) if lpc is not None else None
        if lpc is None and int(end_params[0].hop_length) != int(end_params[1].hop_length):
            raise ValueError(f"{who}: gain at hop {end_params[0].hop_length}, a at hop {end_params[1].hop_length}")
        b_nz = _BranchStage.geometry("fir" if lm is not None else "pass", decoder.noise_filter, (lm,), who)
        if _is_glottal(osc):
            g = StreamGeometry(hop=int(end_params[1].hop_length), phase_hop=int(phase.hop_length),
                               w_hop=int(osc_params[0].hop_length), fir_taps=b_nz.taps, fir_hop=b_nz.hop,
                               window=b_lpc.window if b_lpc else 0, **_GlottalSource.decimator(osc))
            self.source = _GlottalSource(osc, g, B, dev)
            self._end_names = ("gain", "a")
        else:
            self.source = _HarmonicSource(osc, int(phase.hop_length), osc_params, B, dev, False, refuse)
            g = SpectralGeometry(phase_hop=int(phase.hop_length), amp_hop=self.source.amp_hop, noise=b_nz, end=b_lpc)
            self._end_names = ("end filter track",) * len(end_params)
        self.who, self.B, self.geometry, self.checks_first, self._dev = who, B, g, checks_first, dev
        self.noise = _Noise(B, dev, noise is not None, generated_noise)
        self.noise_filter = _BranchStage(b_nz, decoder.noise_filter, self.noise.out, B, dev)
        if lpc is None:
            self.lpc = _AllPoleStage(g.hop, int(end_params[1].shape[2]), B, dev)
        else:   # its input: the running sum osc + filtered noise, as far as both are known
            self.mix = _Track()
            self.lpc = _BranchStage(b_lpc, lpc, self.mix, B, dev)
        self.room = _Room(decoder.room_filter, B, dev) if _room_kind(decoder.room_filter) == "lti" else None
        self.emitted = 0

    def check(self, phase, osc_params, end_params, lm, noise) -> None:
        g, src = self.geometry, self.source
        hop = g.hop if isinstance(g, StreamGeometry) else g.end.hop
        want = [(phase, g.phase_hop, "phase")]
        if src.rows_hop:
            want.append((osc_params[0], src.rows_hop, src.rows_name))
        want += [(t, hop, name) for t, name in zip(end_params, self._end_names)]
        if lm is not None:
            want.append((lm, self.noise_filter.b.hop, "log_mag"))
        if noise is not None:
            want.append((noise, 1, "noise"))
        _check_tracks(want, self.B, self.who)
        src.check(osc_params, self.who)
        self.lpc.check(end_params, self.who)
        self.noise_filter.check((lm,), self.who)
        self.noise.check(noise, self.who)

    def append(self, phase, osc_params, end_params, lm, noise) -> None:
        self.source.append(phase, None, osc_params)
        self.lpc.append(end_params)
        self.noise.append(noise)
        self.noise_filter.append((lm,))

    def _open_lengths(self) -> Tuple[int, int, int, int, int]:
        g, src = self.geometry, self.source
        if isinstance(g, StreamGeometry):
            return _series_open(g, src.ph.end, src.w.end, self.noise.pushed, self.noise_filter.n_ctrl, *self.lpc.ctrl())
        return _spectral_open(g, src.ph.end, src.rows(), self.noise.pushed, self.noise_filter.ctrl(), self.lpc.ctrl())

    def _final_lengths(self) -> dict:
        g, src = self.geometry, self.source
        if not isinstance(g, StreamGeometry):
            src.check_final(self.who)
            return spectral_final_lengths(g, src.ph.end, src.rows(), self.noise.pushed, self.noise_filter.ctrl(),
                                          self.lpc.ctrl())
        n_gain, n_a = self.lpc.ctrl()
        if self.checks_first:
            self.lpc.check_final(self.who)
            src.check_final(self.who)
        fl = final_lengths(g, src.ph.end, self.noise.pushed, self.noise_filter.n_ctrl, min(n_gain, n_a))
        self.lpc.check_final(self.who)
        src.check_final(self.who)
        return fl

    def advance(self, final: bool) -> torch.Tensor:
        g, src, nzf, lpc = self.geometry, self.source, self.noise_filter, self.lpc
        if final:
            fl = self._final_lengths()
            nseg, n_osc, n_noise, n_nz, E = 0, fl["osc"], fl["noise"], fl["noise_filter"], fl["out"]
            n_mix = fl.get("filter_in")
        else:
            fl = None
            nseg, n_osc, n_noise, n_nz, E = self._open_lengths()
            n_mix = min(n_osc, n_nz)
        src.run(nseg, n_osc, final)
        self.noise.run(n_noise)
        nzf.run(n_noise, final, dict(out=n_nz) if final else None)
        if g.window:
            if n_mix > self.mix.end:
                self.mix.append(_take_sum(src.out, nzf.out, self.mix.end, n_mix), fresh=True)
            lpc.run(n_mix, final, fl, self.who)
        lo = self.emitted
        if E <= lo:
            return torch.empty(self.B, 0, device=self._dev)
        if g.window:
            y = lpc.out.get(lo, E)
            lpc.out.drop_before(E)
        else:
            y = lpc.run(_take_sum(src.out, nzf.out, lo, E), lo, E, final)
        self.emitted = E
        return self.room.run(y) if self.room else y


class _Parallel:
    """A branch filter on the source + a branch filter on the noise, summed over the shorter one -> room filter: the
    harmonic-plus-noise decoders.  Built from the tracks of the first push; every push after it passes ``check``, ``append``
    and ``advance`` with the same arguments ``(phase, osc_params, hf_params, nf_params, noise, voicing)``.  ``framewise``:
    the order FramewiseDecoderStream keeps for golf-v1 -- the noise branch runs before the harmonic one, and at finish the
    tracks' own faults are reported before those of the lengths."""

    def __init__(self, who: str, refuse, decoder, kinds, B: int, generated_noise: bool, framewise: bool, phase, osc_params,
                 hf_params, nf_params, noise, voicing):
        dev, P, osc = phase.device, int(phase.hop_length), decoder.harm_oscillator
        if framewise:
            _require_device(phase, who)
        b_harm = _BranchStage.geometry(kinds[0], decoder.harm_filter, hf_params, who, "" if framewise else "harmonic filter ")
        b_nz = _BranchStage.geometry(kinds[1], decoder.noise_filter, nf_params, who, "" if framewise else "noise filter ")
        voiced = voicing is not None
        if _is_glottal(osc):
            g = HPNGeometry(phase_hop=P, source="glottal", w_hop=int(osc_params[0].hop_length), harm=b_harm, noise=b_nz,
                            **_GlottalSource.decimator(osc))
            self.source = _GlottalSource(osc, g, B, dev, voiced)
        else:
            self.source = _HarmonicSource(osc, P, osc_params, B, dev, voiced, refuse)
            g = HPNGeometry(phase_hop=P, source="harmonic", amp_hop=self.source.amp_hop, harm=b_harm, noise=b_nz)
        _require_device(phase, who)
        self.who, self.B, self.geometry, self.framewise, self._dev = who, B, g, framewise, dev
        self.noise = _Noise(B, dev, noise is not None, generated_noise)
        self.harm = self.lpc = _BranchStage(b_harm, decoder.harm_filter, self.source.out, B, dev)   # (lpc: golf-v1's)
        self.noise_filter = _BranchStage(b_nz, decoder.noise_filter, self.noise.out, B, dev)
        self.room = _Room(decoder.end_filter, B, dev) if _room_kind(decoder.end_filter) == "lti" else None
        self.emitted = 0

    def check(self, phase, osc_params, hf_params, nf_params, noise, voicing) -> None:
        g, src = self.geometry, self.source
        want = [(phase, g.phase_hop, "phase")]
        if voicing is not None:
            want.append((voicing, g.phase_hop, "voicing"))
        if src.rows_hop:
            want.append((osc_params[0], src.rows_hop, src.rows_name))
        for b, params, role in ((g.harm, hf_params, "harmonic filter"), (g.noise, nf_params, "noise filter")):
            want += [(t, b.hop, f"{role} track") for t in params]
        if noise is not None:
            want.append((noise, 1, "noise"))
        _check_tracks(want, self.B, self.who)
        src.check(osc_params, self.who)
        self.harm.check(hf_params, self.who)
        self.noise_filter.check(nf_params, self.who)
        self.noise.check(noise, self.who)
        if (voicing is None) == src.voiced:
            raise ValueError(f"{self.who}.push: pass voicing= in every push or in none")

    def append(self, phase, osc_params, hf_params, nf_params, noise, voicing) -> None:
        self.source.append(phase, voicing, osc_params)
        self.noise.append(noise)
        self.harm.append(hf_params)
        self.noise_filter.append(nf_params)

    def advance(self, final: bool) -> torch.Tensor:
        g, src, harm, nzf = self.geometry, self.source, self.harm, self.noise_filter
        n_phase, n_src = src.ph.end, src.rows()
        hc, nc = harm.ctrl(), nzf.ctrl()
        if final:
            if self.framewise:
                harm.check_final(self.who)
            src.check_final(self.who)
            fl = hpn_final_lengths(g, n_phase, n_src, self.noise.pushed, hc, nc)
            nseg, n_osc, n_noise, E = 0, fl["source"], fl["noise"], fl["out"]
            fin_h, fin_n = fl["harm"], fl["noise_branch"]
        else:
            fin_h = fin_n = None
            nseg, n_osc = _source_open(g, n_phase, n_src)
            n_noise = _noise_len(_source_len(g, n_phase, n_src), self.noise.pushed)
            E = min(_branch_open(g.harm, n_osc, hc)[0], _branch_open(g.noise, n_noise, nc)[0])   # (hpn_emit_count)
        src.run(nseg, n_osc, final)
        self.noise.run(n_noise)
        if self.framewise:
            nzf.run(n_noise, final, fin_n, self.who)
        harm.run(n_osc, final, fin_h, self.who)
        if not self.framewise:
            nzf.run(n_noise, final, fin_n, self.who)
        lo = self.emitted
        if E <= lo:
            return torch.empty(self.B, 0, device=self._dev)
        y = _take_sum(harm.out, nzf.out, lo, E)
        self.emitted = E
        return self.room.run(y) if self.room else y


# ---- what a stream accepts -----------------------------------------------------------------------------------------------------
def _plain(obj, cls) -> bool:
    """An instance of ``cls`` that runs ``cls``'s own forward."""
    return isinstance(obj, cls) and type(obj).forward is cls.forward


def _is_glottal(osc) -> bool:
    from .synth import IndexedGlottalFlowTable

    return _plain(osc, IndexedGlottalFlowTable)


def _branch_kind(f) -> Optional[str]:
    """"pass" / "fir" / "frames" / "stft" for PassThrough, the plain zero-phase FIR, the frame-wise LPC filter and the
    STFT-domain filters (LTVCepFilter, LTVMLSAFilter2, DiffWorldSPFilter); None otherwise."""
    from .ctrl import PassThrough
    from .filters import DiffWorldSPFilter, LTVCepFilter, LTVMinimumPhaseFilter, LTVMLSAFilter2, LTVZeroPhaseFIRFilter

    if type(f) is PassThrough:
        return "pass"
    if _plain(f, LTVZeroPhaseFIRFilter):
        return "fir"
    if type(f) in (LTVCepFilter, LTVMLSAFilter2, DiffWorldSPFilter):
        return "stft"
    return "frames" if type(f) is LTVMinimumPhaseFilter else None


def _stft_unsupported(f) -> Optional[str]:
    """What golf_stft_filter_frames_stream_f32 does not take of an STFT-domain filter module, or None."""
    n, hop = int(f.n_fft), int(f.hop_length)
    if not getattr(f, "center", True):
        return f"{type(f).__name__} with center=False"
    if n & (n - 1) or not 64 <= n <= 2048:
        return f"{type(f).__name__} with n_fft {n} (a power of two in [64, 2048] is needed)"
    if n < 2 * hop:
        return f"{type(f).__name__} with n_fft {n} < 2*hop {2 * hop}"
    return None


def _room_kind(f) -> Optional[str]:
    """"pass" / "lti" for PassThrough and the plain LTI room filter; None otherwise."""
    from .ctrl import PassThrough
    from .filters import LTIAcousticFilter

    if type(f) is PassThrough:
        return "pass"
    return "lti" if _plain(f, LTIAcousticFilter) else None


def _value_independent(gen) -> bool:
    """A noise generator whose output does not depend on its reference's values: it can be replaced by pushed noise."""
    from .noise import NoiseBand, SignFlipNoise, UniformNoise

    return not (isinstance(gen, (UniformNoise, SignFlipNoise, NoiseBand)) or getattr(gen, "uses_reference_values", True))


# ---- the public classes --------------------------------------------------------------------------------------------------------
class _Stream:
    """The protocol the three streams share.  A subclass checks its decoder in ``__init__``, parses ``push`` into the
    arguments of its wiring and builds that wiring in ``_open`` from the tracks of the first push."""
    _COVERS = ""

    def __init__(self, decoder, batch_size: int):
        from .noise import StandardNormalNoise

        if int(batch_size) < 1:
            raise ValueError(f"{self._who}: batch_size={batch_size}")
        self.decoder = decoder
        self.B = int(batch_size)
        self.generated_noise = isinstance(decoder.noise_generator, StandardNormalNoise)
        self.geometry = None   # fixed by the first push
        self._pipe = None
        self.finished = False

    @property
    def _who(self) -> str:
        return type(self).__name__

    def _refuse(self, what: str):
        raise NotImplementedError(f"{self._who}: {what} is not supported ({self._COVERS})")

    @property
    def emitted(self) -> int:
        return self._pipe.emitted if self._pipe is not None else 0

    @property
    def latency(self) -> int:
        if self._pipe is None:
            raise RuntimeError(f"{self._who}.latency: the hops are fixed by the first push")
        g = self.geometry
        if isinstance(g, SpectralGeometry):
            return spectral_stream_latency(g)
        return stream_latency(g) if isinstance(g, StreamGeometry) else hpn_stream_latency(g)

    def _geometry(self):
        return self._pipe.geometry

    def _begin_push(self, noise_generator_params, voicing=None) -> None:
        if self.finished:
            raise RuntimeError(f"{self._who}: push after finish()")
        if voicing is not None:
            self._refuse("voicing")
        if len(noise_generator_params):
            self._refuse("noise generator parameters")

    def _push(self, tracks, noise, args) -> torch.Tensor:
        if torch.is_grad_enabled() and any(t.requires_grad for t in tracks if t is not None):
            self._refuse("an input that requires grad (streaming is inference only)")
        if noise is None and not self.generated_noise:
            raise ValueError(f"{self._who}.push: the noise generator {type(self.decoder.noise_generator).__name__} cannot "
                             "run block by block: pass noise= with every push")
        if self._pipe is None:
            self._pipe = self._open(*args)
            self.geometry = self._geometry()
        self._pipe.check(*args)
        with torch.no_grad():
            self._pipe.append(*args)
            return self._pipe.advance(final=False)

    def finish(self) -> torch.Tensor:
        """The inputs have ended: the remaining samples, edges as the one-shot call treats them."""
        if self.finished:
            raise RuntimeError(f"{self._who}: finish() twice")
        self.finished = True
        if self._pipe is None:
            return torch.empty(self.B, 0)
        with torch.no_grad():
            return self._pipe.advance(final=True)

    def _golf_counts(self) -> dict:
        """Steps pushed so far per track (host integers)."""
        p = self._pipe
        n_gain, n_a = p.lpc.ctrl()
        return dict(phase=p.source.n_phase_pushed, wsel=p.source.rows(), noise=None if self.generated_noise else p.noise.pushed,
                    log_mag=p.noise_filter.n_ctrl, gain=n_gain, a=n_a)


class DecoderStream(_Stream):
    """Block-by-block synthesis with a GOLF-ss ``SourceFilterSynth`` (see the module docstring and INTEGRATION.md).

    ``push(phase, harm_oscillator_params=(wsel,), noise_filter_params=(log_mag,), end_filter_params=(gain, a), noise=None)``
    takes AudioTensors holding the next slice of each track (hops as in the one-shot call) and returns a (B, n) fp32 tensor,
    n a multiple of the LPC hop; ``finish()`` returns the remainder.  ``noise=None`` draws N(0,1) on the device as
    StandardNormalNoise does; a decoder with another (value-independent) noise source needs ``noise`` in every push.
    ``latency`` (after the first push, which fixes the hops) is the worst-case lookahead in samples (``stream_latency``).
    Inference only; one stream for the whole batch (no per-row reset)."""
    _COVERS = ("streaming covers the golf-ss decoder: SourceFilterSynth with an indexed glottal table, standard normal noise, "
               "the zero-phase FIR noise filter or none, the sample-wise end filter, the LTI room filter or none")

    def __init__(self, decoder, batch_size: int):
        from .filters import LTVMinimumPhaseFilter, LTVMinimumPhaseFilterPrecise
        from .sf import SourceFilterSynth

        if not _plain(decoder, SourceFilterSynth):
            self._refuse(type(decoder).__name__)
        if decoder.subtract_harmonics:
            self._refuse("subtract_harmonics=True")
        if not _is_glottal(decoder.harm_oscillator):
            self._refuse(f"the oscillator {type(decoder.harm_oscillator).__name__}")
        if not _value_independent(decoder.noise_generator):
            self._refuse(f"the noise generator {type(decoder.noise_generator).__name__}")
        if _branch_kind(decoder.noise_filter) not in ("pass", "fir"):
            self._refuse(f"the noise filter {type(decoder.noise_filter).__name__}")
        ef = decoder.end_filter
        if type(ef) is not LTVMinimumPhaseFilterPrecise:
            self._refuse(f"the end filter {type(ef).__name__}"
                         + (" (the frame-wise end filter)" if isinstance(ef, LTVMinimumPhaseFilter) else ""))
        if _room_kind(decoder.room_filter) is None:
            self._refuse(f"the room filter {type(decoder.room_filter).__name__}")
        super().__init__(decoder, batch_size)
        self.has_fir = _branch_kind(decoder.noise_filter) == "fir"

    counts = _Stream._golf_counts

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), noise_filter_params: Tuple[AudioTensor, ...] = (),
             end_filter_params: Tuple[AudioTensor, ...] = (), noise: AudioTensor = None, voicing=None,
             **other_params) -> torch.Tensor:
        self._begin_push(noise_generator_params, voicing)
        if len(harm_oscillator_params) != 1:
            self._refuse(f"{len(harm_oscillator_params)} oscillator parameters (phase offsets)")
        if len(end_filter_params) != 2 or len(noise_filter_params) != (1 if self.has_fir else 0):
            raise ValueError("DecoderStream.push: end_filter_params=(gain, a) and noise_filter_params=(log_mag,) (or () "
                             "without a noise filter) are required")
        lm = noise_filter_params[0] if self.has_fir else None
        return self._push((phase, *harm_oscillator_params, *end_filter_params, lm, noise), noise,
                          (phase, harm_oscillator_params, end_filter_params, lm, noise))

    def _open(self, *args) -> _Series:
        return _Series(self._who, self.decoder, None, self.B, self.generated_noise, False, *args)


class FramewiseDecoderStream(_Stream):
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
    golf-v1 runs on the wiring of ``HarmonicPlusNoiseStream``.  Inference only; one stream for the whole batch."""
    _COVERS = ("frame-wise streaming covers golf-ff -- SourceFilterSynth with an indexed glottal table, standard normal noise, "
               "the zero-phase FIR noise filter or none, the centred frame-wise end filter LTVMinimumPhaseFilter, the LTI room "
               "filter or none -- and golf-v1 -- HarmonicPlusNoiseSynth with an indexed glottal table, the centred frame-wise "
               "filter on it, the zero-phase FIR noise filter or none, the LTI room filter or none")

    def __init__(self, decoder, batch_size: int):
        from .sf import HarmonicPlusNoiseSynth, SourceFilterSynth

        if _plain(decoder, SourceFilterSynth):
            self.hpn = False
            if decoder.subtract_harmonics:
                self._refuse("subtract_harmonics=True")
            lpc, rf, role = decoder.end_filter, decoder.room_filter, "end filter"
        elif _plain(decoder, HarmonicPlusNoiseSynth):
            self.hpn = True
            lpc, rf, role = decoder.harm_filter, decoder.end_filter, "harmonic filter"
        else:
            self._refuse(type(decoder).__name__)
        if not _is_glottal(decoder.harm_oscillator):
            self._refuse(f"the oscillator {type(decoder.harm_oscillator).__name__}")
        if not _value_independent(decoder.noise_generator):
            self._refuse(f"the noise generator {type(decoder.noise_generator).__name__}")
        if _branch_kind(decoder.noise_filter) not in ("pass", "fir"):
            self._refuse(f"the noise filter {type(decoder.noise_filter).__name__}")
        if _branch_kind(lpc) != "frames":
            self._refuse(f"the {role} {type(lpc).__name__}")
        if not lpc.centred:
            self._refuse("the frame-wise filter with centred=False")
        if _room_kind(rf) is None:
            self._refuse(f"the room filter {type(rf).__name__}")
        super().__init__(decoder, batch_size)
        self.has_fir = _branch_kind(decoder.noise_filter) == "fir"
        self._lpc = lpc

    counts = _Stream._golf_counts

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), noise_filter_params: Tuple[AudioTensor, ...] = (),
             end_filter_params: Tuple[AudioTensor, ...] = (), harm_filter_params: Tuple[AudioTensor, ...] = (),
             noise: AudioTensor = None, voicing=None, **other_params) -> torch.Tensor:
        self._begin_push(noise_generator_params, voicing)
        if len(harm_oscillator_params) != 1:
            self._refuse(f"{len(harm_oscillator_params)} oscillator parameters (phase offsets)")
        lpc_params, other = (harm_filter_params, end_filter_params) if self.hpn else (end_filter_params, harm_filter_params)
        name = "harm_filter_params" if self.hpn else "end_filter_params"
        if len(lpc_params) != 2 or len(other) or len(noise_filter_params) != (1 if self.has_fir else 0):
            raise ValueError(f"FramewiseDecoderStream.push: {name}=(gain, a) and noise_filter_params=(log_mag,) (or () "
                             "without a noise filter) are required")
        if self.hpn:
            args = (phase, harm_oscillator_params, lpc_params, noise_filter_params, noise, None)
            return self._push((phase, *harm_oscillator_params, *lpc_params, *noise_filter_params, noise), noise, args)
        lm = noise_filter_params[0] if self.has_fir else None
        return self._push((phase, *harm_oscillator_params, *lpc_params, lm, noise), noise,
                          (phase, harm_oscillator_params, lpc_params, lm, noise))

    def _open(self, *args):
        if not self.hpn:
            return _Series(self._who, self.decoder, self._lpc, self.B, self.generated_noise, True, *args)
        kinds = ("frames", "fir" if self.has_fir else "pass")
        return _Parallel(self._who, self._refuse, self.decoder, kinds, self.B, self.generated_noise, True, *args)

    def _geometry(self) -> StreamGeometry:
        """The ``StreamGeometry`` of ``emit_count`` / ``final_lengths`` / ``stream_latency`` for this stream."""
        g = self._pipe.geometry
        if not self.hpn:
            return g
        return StreamGeometry(hop=g.harm.hop, phase_hop=g.phase_hop, os=g.os, half=g.half, w_hop=g.w_hop,
                              fir_taps=g.noise.taps, fir_hop=g.noise.hop, window=g.harm.window, hpn=True)


class HarmonicPlusNoiseStream(_Stream):
    """Block-by-block synthesis with a ``HarmonicPlusNoiseSynth`` (module docstring, INTEGRATION.md "Streaming synthesis"):

        ``push(phase, harm_oscillator_params=..., harm_filter_params=..., noise_filter_params=..., noise=None, voicing=None)``

    with the one-shot call's arguments sliced: ``harm_oscillator_params`` (amplitudes,) for HarmonicOscillator,
    AdditiveSynthesizer and V1AdditiveSynthesizer, () for SawToothOscillator and AdditivePulseTrain, (wsel,) for the glottal
    table; each branch's params () / (log_mag,) / (gain, a) / (ceps,) or (mel_sp,) for PassThrough / LTVZeroPhaseFIRFilter /
    LTVMinimumPhaseFilter / the STFT-domain filters LTVCepFilter or DiffWorldSPFilter (NHV: ``harm_filter_params=(ceps,)``);
    ``voicing`` (at the phase's hop) multiplies the phase as the one-shot does.  Same contract as ``DecoderStream``: each push
    returns the (B, n) fp32 samples the inputs pushed so far determine (``hpn_emit_count``), ``finish()`` the rest;
    ``latency`` and ``counts()`` as there.  ``open_stream`` returns this class for a decoder with an STFT-domain branch (NHV)
    only: open it explicitly otherwise.
    Inference only; one stream for the whole batch."""
    _COVERS = ("it covers HarmonicPlusNoiseSynth with the harmonic oscillator bank -- HarmonicOscillator, AdditiveSynthesizer, "
               "V1AdditiveSynthesizer, SawToothOscillator, AdditivePulseTrain -- or an indexed glottal table; PassThrough, "
               "LTVZeroPhaseFIRFilter, LTVMinimumPhaseFilter, LTVCepFilter, LTVMLSAFilter2 or DiffWorldSPFilter (centred, n_fft a power of two "
               "in [64, 2048]) on each branch; standard normal noise or noise pushed with "
               "every block; PassThrough or LTIAcousticFilter as the end filter; voicing at the phase's hop")

    def __init__(self, decoder, batch_size: int):
        from .sf import HarmonicPlusNoiseSynth
        from .synth import (AdditivePulseTrain, AdditiveSynthesizer, HarmonicOscillator, SawToothOscillator,
                            V1AdditiveSynthesizer)

        if not _plain(decoder, HarmonicPlusNoiseSynth):
            self._refuse(type(decoder).__name__)
        osc = decoder.harm_oscillator
        if type(osc) in (HarmonicOscillator, AdditiveSynthesizer, V1AdditiveSynthesizer, SawToothOscillator,
                         AdditivePulseTrain):
            self.source = "harmonic"
        elif _is_glottal(osc):
            self.source = "glottal"
        else:
            self._refuse(f"the oscillator {type(osc).__name__}")
        if not _value_independent(decoder.noise_generator):
            self._refuse(f"the noise generator {type(decoder.noise_generator).__name__}")
        self._kinds = {}
        for role, f in (("harmonic filter", decoder.harm_filter), ("noise filter", decoder.noise_filter)):
            self._kinds[role] = _branch_kind(f)
            if self._kinds[role] is None:
                self._refuse(f"the {role} {type(f).__name__}"
                             + (" (the sample-wise LPC filter)" if type(f).__name__ == "LTVMinimumPhaseFilterPrecise" else ""))
            if self._kinds[role] == "stft" and _stft_unsupported(f):
                self._refuse(f"the {role} " + _stft_unsupported(f))
        if _room_kind(decoder.end_filter) is None:
            self._refuse(f"the end filter {type(decoder.end_filter).__name__}")
        super().__init__(decoder, batch_size)

    def counts(self) -> dict:
        """Steps pushed so far per track (host integers)."""
        p = self._pipe
        return dict(phase=p.source.n_phase_pushed, voicing=p.source.vraw.end if p.source.voiced else None,
                    oscillator=p.source.rows(), noise=None if self.generated_noise else p.noise.pushed,
                    harm_filter=p.harm.ctrl(), noise_filter=p.noise_filter.ctrl())

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), harm_filter_params: Tuple[AudioTensor, ...] = (),
             noise_filter_params: Tuple[AudioTensor, ...] = (), noise: AudioTensor = None, voicing: AudioTensor = None,
             **other_params) -> torch.Tensor:
        self._begin_push(noise_generator_params)
        osc = self.decoder.harm_oscillator
        n_osc = 1 if self.source == "glottal" or _HarmonicSource.takes_amplitudes(osc) else 0
        if len(harm_oscillator_params) != n_osc:
            self._refuse(f"{len(harm_oscillator_params)} oscillator parameters for {type(osc).__name__}"
                         f" (it takes {n_osc}; initial_phase / phase_offset are not streamed)")
        want = {"pass": 0, "fir": 1, "frames": 2, "stft": 1}
        for name, params, role in (("harm_filter_params", harm_filter_params, "harmonic filter"),
                                   ("noise_filter_params", noise_filter_params, "noise filter")):
            if len(params) != want[self._kinds[role]]:
                raise ValueError(f"HarmonicPlusNoiseStream.push: {name} must hold {want[self._kinds[role]]} tracks for the "
                                 f"{role} ({self._kinds[role]})")
        if voicing is not None and int(voicing.hop_length) != int(phase.hop_length):
            self._refuse(f"voicing at hop {voicing.hop_length} with the phase at hop {phase.hop_length}")
        args = (phase, harm_oscillator_params, harm_filter_params, noise_filter_params, noise, voicing)
        return self._push((phase, *harm_oscillator_params, *harm_filter_params, *noise_filter_params, noise, voicing), noise,
                          args)

    def _open(self, *args) -> _Parallel:
        kinds = (self._kinds["harmonic filter"], self._kinds["noise filter"])
        return _Parallel(self._who, self._refuse, self.decoder, kinds, self.B, self.generated_noise, False, *args)


class SpectralDecoderStream(_Stream):
    """Block-by-block synthesis with a ``SourceFilterSynth`` on a harmonic source whose end filter works in the STFT domain:
    the WORLD baseline (AdditivePulseTrain + filtered noise -> DiffWorldSPFilter -> room filter).

        ``push(phase, harm_oscillator_params=(), noise_filter_params=(log_mag,), end_filter_params=(mel_sp,), noise=None)``

    with the one-shot call's arguments sliced (``harm_oscillator_params`` (amplitudes,) for the oscillators that take them).
    Same contract as ``DecoderStream``: each push returns the (B, n) fp32 samples the inputs pushed so far determine
    (``spectral_emit_count``), ``finish()`` the rest -- it raises ``GolfError`` for an utterance too short to be
    reflect-padded, as the one-shot does; ``latency`` (``spectral_stream_latency``) and ``counts()`` as there.  Every STFT
    frame is filtered once, by golf_stft_filter_frames_stream_f32, which carries the last ceil(n_fft/hop) - 1 of them.
    Inference only; one stream for the whole batch."""
    _COVERS = ("it covers SourceFilterSynth with the harmonic oscillator bank -- HarmonicOscillator, AdditiveSynthesizer, "
               "V1AdditiveSynthesizer, SawToothOscillator, AdditivePulseTrain --, standard normal noise or noise pushed with "
               "every block, the zero-phase FIR noise filter or none, LTVCepFilter, LTVMLSAFilter2 or DiffWorldSPFilter (centred, n_fft a "
               "power of two in [64, 2048]) as the end filter, the LTI room filter or none")

    def __init__(self, decoder, batch_size: int):
        from .sf import SourceFilterSynth
        from .synth import (AdditivePulseTrain, AdditiveSynthesizer, HarmonicOscillator, SawToothOscillator,
                            V1AdditiveSynthesizer)

        if not _plain(decoder, SourceFilterSynth):
            self._refuse(type(decoder).__name__)
        if decoder.subtract_harmonics:
            self._refuse("subtract_harmonics=True")
        osc, ef = decoder.harm_oscillator, decoder.end_filter
        if type(osc) not in (HarmonicOscillator, AdditiveSynthesizer, V1AdditiveSynthesizer, SawToothOscillator,
                             AdditivePulseTrain):
            self._refuse(f"the oscillator {type(osc).__name__}")
        if not _value_independent(decoder.noise_generator):
            self._refuse(f"the noise generator {type(decoder.noise_generator).__name__}")
        if _branch_kind(decoder.noise_filter) not in ("pass", "fir"):
            self._refuse(f"the noise filter {type(decoder.noise_filter).__name__}")
        if _branch_kind(ef) != "stft":
            self._refuse(f"the end filter {type(ef).__name__}")
        if _stft_unsupported(ef):
            self._refuse("the end filter " + _stft_unsupported(ef))
        if _room_kind(decoder.room_filter) is None:
            self._refuse(f"the room filter {type(decoder.room_filter).__name__}")
        super().__init__(decoder, batch_size)
        self.has_fir = _branch_kind(decoder.noise_filter) == "fir"

    def counts(self) -> dict:
        """Steps pushed so far per track (host integers)."""
        p = self._pipe
        return dict(phase=p.source.n_phase_pushed, oscillator=p.source.rows(),
                    noise=None if self.generated_noise else p.noise.pushed, noise_filter=p.noise_filter.ctrl(),
                    end_filter=p.lpc.ctrl())

    def push(self, phase: AudioTensor, harm_oscillator_params: Tuple[AudioTensor, ...] = (),
             noise_generator_params: Tuple = (), noise_filter_params: Tuple[AudioTensor, ...] = (),
             end_filter_params: Tuple[AudioTensor, ...] = (), noise: AudioTensor = None, voicing=None,
             **other_params) -> torch.Tensor:
        self._begin_push(noise_generator_params, voicing)
        osc = self.decoder.harm_oscillator
        n_osc = 1 if _HarmonicSource.takes_amplitudes(osc) else 0
        if len(harm_oscillator_params) != n_osc:
            self._refuse(f"{len(harm_oscillator_params)} oscillator parameters for {type(osc).__name__}"
                         f" (it takes {n_osc}; initial_phase / phase_offset are not streamed)")
        if len(end_filter_params) != 1 or len(noise_filter_params) != (1 if self.has_fir else 0):
            raise ValueError("SpectralDecoderStream.push: end_filter_params=(controls,) and noise_filter_params=(log_mag,) "
                             "(or () without a noise filter) are required")
        lm = noise_filter_params[0] if self.has_fir else None
        return self._push((phase, *harm_oscillator_params, *end_filter_params, lm, noise), noise,
                          (phase, harm_oscillator_params, end_filter_params, lm, noise))

    def _open(self, *args) -> _Series:
        return _Series(self._who, self.decoder, self.decoder.end_filter, self.B, self.generated_noise, True, *args,
                       refuse=self._refuse)


def open_stream(decoder, batch_size: int):
    """A streaming synthesiser for ``decoder``: ``SpectralDecoderStream`` for a ``SourceFilterSynth`` whose end filter works in
    the STFT domain (WORLD), ``HarmonicPlusNoiseStream`` for a ``HarmonicPlusNoiseSynth`` with such a branch (NHV),
    ``FramewiseDecoderStream`` for the decoders built on the frame-wise LPC filter (golf-ff's end filter, golf-v1's harmonic
    filter), ``DecoderStream`` otherwise (golf-ss)."""
    from .filters import LTVMinimumPhaseFilter
    from .sf import HarmonicPlusNoiseSynth, SourceFilterSynth

    if isinstance(decoder, SourceFilterSynth) and _branch_kind(decoder.end_filter) == "stft":
        return SpectralDecoderStream(decoder, batch_size)
    if isinstance(decoder, HarmonicPlusNoiseSynth) and "stft" in (_branch_kind(decoder.harm_filter),
                                                                  _branch_kind(decoder.noise_filter)):
        return HarmonicPlusNoiseStream(decoder, batch_size)
    if isinstance(decoder, HarmonicPlusNoiseSynth) or isinstance(getattr(decoder, "end_filter", None), LTVMinimumPhaseFilter):
        return FramewiseDecoderStream(decoder, batch_size)
    return DecoderStream(decoder, batch_size)
