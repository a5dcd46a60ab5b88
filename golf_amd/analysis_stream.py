"""Block-by-block analysis: the streaming counterparts of ``f0.F0Analysis``, ``f0.F0Tracker``, ``lpc.LPCAnalysis``,
``lpc.SourceFilterLPCAnalysis``, ``hna.HarmonicNoiseAnalysis``, ``envelope.SpectralEnvelopeAnalysis`` and ``glottal.GlottalSourceAnalysis`` (with its residual,
``functional.ltv_residual``), for a live waveform that feeds a decoder stream (``stream.DecoderStream`` and its siblings take
exactly these tracks).

The protocol is the decoder streams': ``push(x)`` takes the next (B, n) block of the waveform, any n >= 0, and returns the
frames that became final, in the types the module's ``forward`` returns (possibly with zero frames); ``finish()`` ends the
utterance, returns the rest and leaves the stream ready for a new utterance.  Everything pushed out plus ``finish()`` is
``torch.equal`` to the one-shot module on the concatenated input, whatever the cuts.

YIN frames and LPC frames are frame-local: a frame is final once its last sample has come, and the one-shot kernels run
``centred=False, n_frames=`` on the buffered samples that the open frames still need -- a frame's arithmetic does not depend
on where it sits in the row, which is why the result is exact.  Zeros stand before sample 0 and after the end, as the
definitions say.  The tracker is not frame-local: its candidates are, and the path through them is decided ``lag`` frames
late by golf_f0_viterbi_stream_f32 (csrc/f0_viterbi_stream.hip), whose costs are carried from push to push.  The
harmonic-plus-noise analysis takes two inputs, the waveform and its f0 track, which arrive at different paces
(``HarmonicNoiseStream``): its frames are frame-local too, given the f0 of the neighbouring frames.  So are the frames of the
spectral-envelope analysis (``SpectralEnvelopeStream``) and of the glottal-source analysis (``GlottalSourceStream``), and the
samples of the residual it reads (``ResidualStream``): each runs its one-shot kernel at a position of the utterance.

Inference only; one stream for the whole batch; ``push`` does no host-device synchronisation.
"""
from __future__ import annotations

import torch

from . import _lib
from . import functional as GF
from .audiotensor import AudioTensor
from .envelope import SpectralEnvelopeAnalysis
from .f0 import F0Analysis, F0Tracker
from .glottal import GlottalSourceAnalysis
from .hna import HarmonicNoiseAnalysis
from .lpc import LPCAnalysis, SourceFilterLPCAnalysis
from .stream import _Track

__all__ = ["F0Stream", "F0TrackerStream", "LPCAnalysisStream", "SourceFilterLPCStream", "HarmonicNoiseStream",
           "SpectralEnvelopeStream", "GlottalSourceStream", "ResidualStream", "open_analysis_stream", "frames_open", "frames_final", "frame_reach",
           "hna_frames_final", "hna_keep_from", "env_frames_final", "env_keep_from", "res_samples_final", "res_samples_finish",
           "res_keep_from"]


# ---- geometry: host integers only ------------------------------------------------------------------------------------------
def frames_open(n: int, span: int, hop: int, centred: bool) -> int:
    """Frames, counted from index 0, all of whose ``span`` samples lie below ``n``: frame f covers
    ``[origin + f * hop, origin + f * hop + span)`` with origin ``-(span // 2)`` centred and 0 otherwise."""
    room = n - frame_reach(span, centred)
    return room // hop + 1 if room >= 0 else 0


def frames_final(T: int, span: int, hop: int, centred: bool) -> int:
    """Frames of the one-shot analysis of T samples (``functional.f0_frames`` / ``lpc_analysis_frames``)."""
    return GF.lpc_analysis_frames(T, span, hop, centred)


def frame_reach(span: int, centred: bool) -> int:
    """Samples from a frame's own time ``f * hop`` to its end: the latency of a frame-local stream."""
    return span - span // 2 if centred else span


class _Stream:
    """What every analysis stream shares: the constructor's checks, the check of a pushed block, one ``stream._Track`` per
    input -- a buffer along dimension 1 that knows where in the utterance it starts -- and the run loop over them.  A
    subclass implements ``_total(final)``, the units (frames or samples) of the utterance that are final so far;
    ``_keep()``, for each track the position from which the open units still read; and ``_compute(n, final, *how)``, the
    next n units from the tracks."""

    def __init__(self, batch_size: int, hop: int, n_tracks: int):
        if int(batch_size) < 1:
            raise ValueError(f"{self._who}: batch_size={batch_size}")
        self.B, self.hop = int(batch_size), int(hop)
        if self.hop < 1:
            raise _lib.GolfError(f"{self._who}: hop={self.hop} must be >= 1")
        self._tracks = tuple(_Track() for _ in range(n_tracks))
        self._reset()

    @property
    def _who(self) -> str:
        return type(self).__name__

    @property
    def pushed(self) -> int:
        """Samples of this utterance so far."""
        return self._tracks[0].end

    def _reset(self) -> None:
        self._done = 0   # units of this utterance computed so far
        for tr in self._tracks:
            tr.start = 0
            if tr.data is not None:
                tr.data = tr.data[:, :0]

    def _device(self):
        for tr in self._tracks:
            if tr.data is not None:
                return tr.data.device
        return torch.device("cuda")

    def _check_block(self, t, name: str, hop: int, ndim: int = 2) -> torch.Tensor:
        """The checks every pushed block passes before its device is looked at: the hop of an AudioTensor, the shape, no
        gradient; under autocast fp16 / bf16 become fp32."""
        if isinstance(t, AudioTensor):
            assert t.hop_length == hop, f"{name} must be at hop {hop} (got {t.hop_length})"
            t = t.as_tensor()
        if t.dim() != ndim or t.shape[0] != self.B:
            raise ValueError(f"{self._who}.push: {name} of shape {tuple(t.shape)}; the stream has B={self.B}")
        if torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError(f"{self._who}: an input that requires grad (streaming is inference only) is not supported")
        if torch.is_autocast_enabled() and t.is_floating_point():   # as the one-shot functions: fp16 / bf16 become fp32
            t = t.float()
        return t.detach()

    def _take(self, t, name: str, hop: int) -> torch.Tensor:
        t = self._check_block(t, name, hop)
        _lib.require_device(t)
        return t

    def _advance(self, blocks, final: bool, *how):
        """The run loop: each block (or None) goes to the end of its track; the units that became final are computed; then
        the utterance is over, or every track drops what no open unit reads (at most what has come).  Nothing here can
        require grad: ``_check_block`` has detached the blocks, and the kernels' wrappers detach what they take."""
        for tr, t in zip(self._tracks, blocks):
            if t is not None:
                tr.append(t, True)   # fresh: the block is the caller's to give, an emptied track takes it as it is
        n = max(self._total(final) - self._done, 0)
        out = self._compute(n, final, *how)
        self._done += n
        if final:
            self._reset()
        else:
            for tr, lo in zip(self._tracks, self._keep()):
                tr.drop_before(lo)
        return out


class _FrameStream(_Stream):
    """The protocol and the sample track the one-input streams share.  A subclass names its frame (``span``, ``hop``,
    ``centred``) and implements ``_frames(x, k)``, the one-shot call for the first k frames of x with ``centred=False``, and
    ``_emit(k, out, final)``, what the push returns.  The track starts with the zeros before sample 0."""

    def __init__(self, module, batch_size: int, span: int):
        self.module, self.span, self.centred = module, int(span), bool(module.centred)
        self._origin = -(self.span // 2) if self.centred else 0
        super().__init__(batch_size, module.hop_length, 1)

    framed = property(lambda self: self._done, doc="Frames handed to the kernels so far.")

    def _reset(self) -> None:
        super()._reset()
        tr = self._tracks[0]
        tr.start = self._origin
        if tr.data is not None:
            tr.data = tr.data.new_zeros(self.B, -self._origin)

    @property
    def pushed(self) -> int:
        return max(self._tracks[0].end, 0)   # (the zeros before sample 0 are there from the first push on)

    @property
    def latency(self) -> int:
        """The smallest number of samples beyond a frame's own time ``f * hop`` after which it has been emitted."""
        return frame_reach(self.span, self.centred)

    def _total(self, final: bool) -> int:
        return (frames_final if final else frames_open)(self._tracks[0].end, self.span, self.hop, self.centred)

    def _keep(self):
        return (self._origin + self._done * self.hop,)   # the start of the next frame

    def _compute(self, k: int, final: bool):
        """The frames that became final, through the one-shot kernels."""
        out = None
        if k > 0:
            tr = self._tracks[0]   # it starts at the next frame, or ends before it: then only the zeros after the end are read
            x = tr.data if self._origin + self._done * self.hop < tr.end else tr.data.new_zeros(self.B, 1)
            out = self._frames(x, k)
        return self._emit(k, out, final)

    def _run(self, x, final: bool):
        tr = self._tracks[0]
        if x is not None:
            x = self._take(x, "x", 1)
        if tr.data is None:
            tr.data = torch.zeros(self.B, -self._origin, device=self._device()) if x is None else \
                x.new_zeros(self.B, -self._origin)
        if x is not None:   # hop > span: the next frame may start beyond what has come, and the samples before it are dropped
            skip = min(max(self._origin + self._done * self.hop - tr.end, 0), x.shape[1])
            tr.start += skip   # (the track is empty then)
            x = x[:, skip:]
        return self._advance((x,), final)


class _F0Base(_FrameStream):
    def __init__(self, module, batch_size: int, voicing: bool = False):
        super().__init__(module, batch_size, module.window_length + module.tau_max)
        self.voicing = bool(voicing)

    def _wrap(self, out):
        f0 = AudioTensor(out[0], self.hop)
        return (f0, AudioTensor((out[0] > 0).float(), self.hop)) if self.voicing else f0

    def push(self, x):
        """The next block of the waveform -> the f0 of the frames that became final, an ``AudioTensor`` at ``hop_length``
        (with ``voicing=True``: ``(f0, voicing)``)."""
        return self._wrap(self._run(x, False))

    def finish(self):
        """The utterance has ended: the remaining frames; the stream starts a new utterance."""
        return self._wrap(self._run(None, True))

    def push_all(self, x):
        """``push`` with the plain tensors of the module's ``analyse``."""
        return self._run(x, False)

    def finish_all(self):
        return self._run(None, True)


class F0Stream(_F0Base):
    """``F0Analysis`` block by block: ``push`` / ``finish`` give what ``forward`` gives, ``push_all`` / ``finish_all`` the
    ``(f0, period, ap)`` of ``analyse``; ``voicing=True`` returns the voicing track beside f0.  A frame is emitted once its
    last sample has been pushed: ``latency`` samples after its own time."""

    def __init__(self, module: F0Analysis, batch_size: int, voicing: bool = False):
        if not isinstance(module, F0Analysis) or isinstance(module, F0Tracker):
            raise TypeError(f"F0Stream: an F0Analysis is needed (got {type(module).__name__}; F0TrackerStream takes an F0Tracker)")
        super().__init__(module, batch_size, voicing)

    def _frames(self, x, k):
        m = self.module
        return GF.f0_yin(x, m.sample_rate, self.hop, m.f0_min, m.f0_max, m.window_length, m.threshold, m.rms_floor,
                         centred=False, n_frames=k, return_all=True)

    def _emit(self, k, out, final):
        if k > 0:
            return out
        z = torch.empty(self.B, 0, dtype=torch.float32, device=self._device())
        return z, z.clone(), z.clone()


class F0TrackerStream(_F0Base):
    """``F0Tracker`` block by block with a fixed lag: the candidates of a frame are computed once its last sample has come,
    and frame g is decided once frame ``g + lag`` has its candidates, from the best path that ends there
    (``functional.f0_viterbi_stream``); ``finish()`` decides the rest from the last frame.  The result depends on the waveform
    and ``lag`` alone, never on the cuts, and equals ``F0Tracker`` whenever ``lag >= F - 1``.  ``push`` / ``finish`` give what
    ``forward`` gives, ``push_all`` / ``finish_all`` give ``(f0, state)``; ``voicing=True`` returns the voicing track beside
    f0.  ``latency`` is the frame's reach plus ``lag * hop_length`` samples.

    ``lag=8`` is four times the lag from which the fixed-lag path equalled the whole-utterance path on the project's synthetic
    end-to-end cases (80 ms at 24 kHz and hop 240); like the costs, it is not tuned on speech."""

    def __init__(self, module: F0Tracker, batch_size: int, lag: int = 8, voicing: bool = False):
        if not isinstance(module, F0Tracker):
            raise TypeError(f"F0TrackerStream: an F0Tracker is needed (got {type(module).__name__})")
        if not 0 <= int(lag) <= GF.F0_STREAM_MAX_LAG:
            raise _lib.GolfError(f"F0TrackerStream: lag={lag} frames must be 0..{GF.F0_STREAM_MAX_LAG}")
        if not 1 <= int(module.n_candidates) <= GF.F0_MAX_CANDIDATES:
            raise _lib.GolfError(f"F0TrackerStream: n_candidates={module.n_candidates} must be 1..{GF.F0_MAX_CANDIDATES}")
        super().__init__(module, batch_size, voicing)
        self.lag = int(lag)
        self._carry = None

    @property
    def latency(self) -> int:
        return frame_reach(self.span, self.centred) + self.lag * self.hop

    @property
    def decided(self) -> int:
        """Frames of this utterance emitted so far."""
        return GF.f0_viterbi_stream_decided(self.framed, self.lag)

    def _frames(self, x, k):
        m = self.module
        return GF.f0_candidates(x, m.sample_rate, self.hop, m.f0_min, m.f0_max, m.window_length, m.n_candidates, m.rms_floor,
                                centred=False, n_frames=k)

    def _emit(self, k, out, final):
        m, dev = self.module, self._device()
        if self._carry is None:
            self._carry = GF.f0_viterbi_stream_state(self.B, m.n_candidates, self.lag, dev)
        if k > 0:
            period, ap = out
        else:
            period = torch.empty(self.B, 0, m.n_candidates, dtype=torch.float32, device=dev)
            ap = period
        return GF.f0_viterbi_stream(period, ap, self._carry, self.framed, self.lag, m.sample_rate, float(m.tau_min),
                                    m.unvoiced_cost, m.lag_cost, m.jump_cost, m.switch_cost, flush=final, return_state=True)


class _LPCStream(_FrameStream):
    """What the two LPC streams share: frames of ``window_length`` samples and the protocol over the tuple ``(gain, a, ...)``.
    A subclass implements ``_frames(x, k)`` and ``_widths()``, the last dimension of each result after ``gain``."""

    def __init__(self, module, batch_size: int, return_rc: bool):
        super().__init__(module, batch_size, module.window_length)
        self.return_rc = bool(return_rc)

    def _emit(self, k, out, final):
        if k > 0:
            return out
        dev = self._device()
        return (torch.empty(self.B, 0, dtype=torch.float32, device=dev),) + tuple(
            torch.empty(self.B, 0, n, dtype=torch.float32, device=dev) for n in self._widths())

    def push_all(self, x):
        return self._run(x, False)

    def finish_all(self):
        return self._run(None, True)

    def push(self, x):
        """The next block of the waveform -> ``(gain, a)`` (``(gain, a, rc)``) of the frames that became final, AudioTensors
        at ``hop_length``."""
        return tuple(AudioTensor(t, self.hop) for t in self._run(x, False))

    def finish(self):
        """The utterance has ended: the remaining frames; the stream starts a new utterance."""
        return tuple(AudioTensor(t, self.hop) for t in self._run(None, True))


class LPCAnalysisStream(_LPCStream):
    """``LPCAnalysis`` block by block: ``push`` / ``finish`` give ``(gain, a)`` as ``forward`` does -- the
    ``end_filter_params`` of a decoder stream -- and with ``return_rc=True`` ``(gain, a, rc)``; ``push_all`` / ``finish_all``
    give the plain tensors of ``analyse``.  A frame is emitted once its last sample has been pushed."""

    def __init__(self, module: LPCAnalysis, batch_size: int, return_rc: bool = False):
        if not isinstance(module, LPCAnalysis):
            raise TypeError(f"LPCAnalysisStream: an LPCAnalysis is needed (got {type(module).__name__})")
        super().__init__(module, batch_size, return_rc)

    def _frames(self, x, k):
        m = self.module
        return GF.lpc_analysis(x, m._window, self.hop, m.lpc_order, centred=False, n_frames=k, return_rc=self.return_rc)

    def _widths(self):
        return (self.module.lpc_order,) * (2 if self.return_rc else 1)


class SourceFilterLPCStream(_LPCStream):
    """``SourceFilterLPCAnalysis`` block by block, with the protocol of ``LPCAnalysisStream``: ``push`` / ``finish`` give
    ``(gain, a)``, then ``rc`` with ``return_rc=True`` and ``source`` with ``return_source=True``, AudioTensors at
    ``hop_length``; ``push_all`` / ``finish_all`` give the plain tensors of ``analyse``.  Its frames are frame-local like the
    plain analysis', so everything pushed out plus ``finish()`` is ``torch.equal`` to the module on the concatenated input,
    whatever the cuts, and ``(gain, a)`` feed a ``ResidualStream`` in ``LPCAnalysisStream``'s place."""

    def __init__(self, module: SourceFilterLPCAnalysis, batch_size: int, return_rc: bool = False, return_source: bool = False):
        if not isinstance(module, SourceFilterLPCAnalysis):
            raise TypeError(f"SourceFilterLPCStream: a SourceFilterLPCAnalysis is needed (got {type(module).__name__})")
        super().__init__(module, batch_size, return_rc)
        self.return_source = bool(return_source)

    def _frames(self, x, k):
        m = self.module
        return GF.source_filter_lpc(x, m._window, self.hop, m.lpc_order, m.source_order, m.iterations, m.preemphasis,
                                    centred=False, n_frames=k, return_rc=self.return_rc, return_source=self.return_source)

    def _widths(self):
        m = self.module
        return (m.lpc_order,) * (2 if self.return_rc else 1) + ((m.source_order,) if self.return_source else ())


# ---- harmonic-plus-noise analysis: two inputs at two paces ------------------------------------------------------------------
def hna_frames_final(pushed: int, f0_received: int, span: int, hop: int) -> int:
    """Frames of a ``HarmonicNoiseStream``, counted from index 0, that are final after ``pushed`` samples and ``f0_received``
    f0 frames: frame f is final once the longest window it can take (``span = max(max_window, unvoiced_window)`` samples
    centred on ``f * hop``) lies below ``pushed`` and f0 frame ``f + 1``, the chirp's next neighbour, has come."""
    return min(frames_open(pushed, span, hop, True), max(f0_received - 1, 0))


def hna_keep_from(next_frame: int, span: int, hop: int):
    """``(sample, f0 frame)`` from which a ``HarmonicNoiseStream`` whose next frame is ``next_frame`` keeps its inputs: the
    start of that frame's longest window, and its previous neighbour."""
    return max(next_frame * hop - span // 2, 0), max(next_frame - 1, 0)


class _AudioF0Stream(_Stream):
    """The protocol of the streams that take a waveform and a frame-rate f0 track at two paces, one track each.  A subclass
    names its module type, sets ``span`` and implements ``_total(final)``, the frames final so far; ``_keep()``, the
    ``(sample, f0 frame)`` from which the open frames still read; and ``_frames(x, f0, x_t0, f_first, f0_first, k, last,
    full)``, frames ``f_first .. f_first + k - 1`` from the buffers, which start at sample ``x_t0`` and frame ``f0_first``."""

    _module_type = None
    _audio = "x"   # the name of the waveform argument in messages

    def __init__(self, module, batch_size: int):
        if not isinstance(module, self._module_type):
            a = self._module_type.__name__
            raise TypeError(f"{self._who}: a{'n' if a[0] in 'AEIOU' else ''} {a} is needed (got {type(module).__name__})")
        self.module = module
        super().__init__(batch_size, module.hop_length, 2)

    f0_received = property(lambda self: self._tracks[1].end, doc="f0 frames of this utterance so far.")
    framed = property(lambda self: self._done, doc="Frames emitted so far.")

    def _compute(self, k: int, final: bool, full: bool):
        x, f0 = self._tracks
        xb = x.data if x.data is not None else torch.empty(self.B, 0, dtype=torch.float32, device=self._device())
        fb = f0.data if f0.data is not None else torch.empty(self.B, 0, dtype=torch.float32, device=self._device())
        return self._frames(xb, fb, x.start, self._done, f0.start, k, final, full)

    def _run(self, x, f0, final: bool, full: bool):
        x = None if x is None else self._take(x, self._audio, 1)
        f0 = None if f0 is None else self._take(f0, "f0", self.hop)
        return self._advance((x, f0), final, full)


class HarmonicNoiseStream(_AudioF0Stream):
    """``hna.HarmonicNoiseAnalysis`` block by block, for live audio and its live f0 (an ``F0Stream`` or ``F0TrackerStream``
    on the same audio, which is ``lag`` frames late) feeding a ``stream.HarmonicPlusNoiseStream``.

    ``push(x=None, f0=None)`` takes the next (B, n) block of the waveform (a tensor or an ``AudioTensor`` at hop 1) and / or the
    next (B, k) f0 frames (a tensor or an ``AudioTensor`` at ``hop_length``); either may be absent or empty.  It returns the
    frames that became final in the types of ``forward``: ``(amplitudes, log_mag)``, AudioTensors at ``hop_length``, or
    ``amplitudes`` alone when ``n_mag`` is None, possibly with zero frames.  ``finish()`` ends the utterance -- F = the f0
    frames received, T = the samples received; frames beyond T read zeros and audio beyond the last frame's window is
    ignored, as the one-shot does for the same ``(x, f0)`` -- returns the rest and starts a new utterance.  ``push_all`` /
    ``finish_all`` return the plain tensors of ``analyse``, with the phases.  Everything pushed out plus ``finish()`` is
    ``torch.equal`` to the module on the concatenated ``(x, f0)``, for any cuts of either input and any interleaving.

    Frame f is final once ``pushed >= f * hop + frame_reach(Lmax, True)``, ``Lmax = max(max_window, unvoiced_window)``, and f0
    frame ``f + 1`` has come (``hna_frames_final``): the rule is the worst case over the batch and over the window lengths,
    so ``push`` never reads the device.  The frames run through golf_harmonic_analysis_stream_f32, the one-shot kernel at a
    position of the utterance.  Samples before ``next_frame * hop - Lmax // 2`` and f0 frames before ``next_frame - 1`` are
    dropped (``hna_keep_from``); whichever input runs ahead is held until the other catches up.

    ``latency`` is the audio side, ``frame_reach(Lmax, True)`` samples beyond a frame's own time (1024 at the defaults); with
    the f0 source the whole figure is ``max(latency, hop_length + the f0 stream's latency)``: 240 + 2520 = 2760 samples at the
    recipe behind ``F0TrackerStream(lag=8)``.

    Inference only; one stream for the whole batch; ``push`` does no host-device synchronisation."""

    _module_type = HarmonicNoiseAnalysis

    def __init__(self, module: HarmonicNoiseAnalysis, batch_size: int):
        super().__init__(module, batch_size)
        self.span = max(int(module.max_window), int(module.unvoiced_window))   # Lmax

    @property
    def latency(self) -> int:
        """The smallest number of samples beyond a frame's own time ``f * hop`` after which it can have been emitted: the
        audio side.  The f0 side adds to it: the frame needs f0 frame ``f + 1`` (class docstring)."""
        return frame_reach(self.span, True)

    def _total(self, final: bool) -> int:
        # finish(): one frame per f0 frame, whatever the number of samples
        x, f0 = self._tracks
        return f0.end if final else hna_frames_final(x.end, f0.end, self.span, self.hop)

    def _keep(self):
        return hna_keep_from(self._done, self.span, self.hop)

    def _frames(self, x, f0, x_t0: int, f_first: int, f0_first: int, k: int, last: bool, phases: bool):
        """Frames ``f_first .. f_first + k - 1`` from the buffers, which start at sample ``x_t0`` and frame ``f0_first``."""
        m = self.module
        return GF.harmonic_analysis_stream(x, f0, x_t0, f_first, f0_first, k, last, m.sample_rate, self.hop, m.num_harmonics,
                                           m.n_mag, m.periods, m.min_window, m.max_window, m.unvoiced_window, m.smooth, m.eps,
                                           return_phases=phases)

    def _wrap(self, out):
        if self.module.n_mag is None:
            return AudioTensor(out, self.hop)
        return AudioTensor(out[0], self.hop), AudioTensor(out[1], self.hop)

    def push(self, x=None, f0=None):
        """The next block of the waveform and / or the next f0 frames -> the frames that became final, as ``forward``
        returns them."""
        return self._wrap(self._run(x, f0, False, False))

    def finish(self):
        """The utterance has ended: the remaining frames; the stream starts a new utterance."""
        return self._wrap(self._run(None, None, True, False))

    def push_all(self, x=None, f0=None):
        """``push`` with the plain tensors of the module's ``analyse``: ``(amplitudes, phases[, log_mag])``."""
        return self._run(x, f0, False, True)

    def finish_all(self):
        return self._run(None, None, True, True)


# ---- spectral-envelope analysis: a frame reads its own f0 and the samples within hwmax of its centre ------------------------
def env_frames_final(pushed: int, f0_received: int, hwmax: int, hop: int) -> int:
    """Frames of a ``SpectralEnvelopeStream``, counted from index 0, that are final after ``pushed`` samples and
    ``f0_received`` f0 frames: frame f is final once the longest window it can take (``hwmax`` samples either side of
    ``f * hop``) lies below ``pushed``, that is ``f * hop + hwmax + 1 <= pushed``, and its own f0 frame has come."""
    room = pushed - hwmax - 1
    return min(room // hop + 1 if room >= 0 else 0, f0_received)


def env_keep_from(next_frame: int, hwmax: int, hop: int):
    """``(sample, f0 frame)`` from which a ``SpectralEnvelopeStream`` whose next frame is ``next_frame`` keeps its inputs."""
    return max(next_frame * hop - hwmax, 0), next_frame


class SpectralEnvelopeStream(_AudioF0Stream):
    """``envelope.SpectralEnvelopeAnalysis`` block by block, for live audio and its live f0 (an ``F0Stream`` or
    ``F0TrackerStream`` on the same audio) feeding the NHV decoder's stream (``stream.HarmonicPlusNoiseStream`` takes ``ceps``
    as the harmonic filter's control).

    ``push(x=None, f0=None)`` takes the next (B, n) block of the waveform and / or the next (B, k) f0 frames, as
    ``HarmonicNoiseStream`` does, and returns the frames that became final as ``forward`` returns them: ``ceps``, an
    AudioTensor at ``hop_length`` (``log_env`` when ``filter_order`` is None), possibly with zero frames.  ``finish()`` ends
    the utterance -- one frame per f0 frame received, T = the samples received -- returns the rest and starts a new utterance.
    ``push_all`` / ``finish_all`` return the plain ``(log_env, ceps)`` of ``analyse``.  Everything pushed out plus
    ``finish()`` is ``torch.equal`` to the module on the concatenated ``(x, f0)``, for any cuts and any interleaving.

    Frame f is final once ``pushed >= f * hop + hwmax + 1``, ``hwmax = floor(1.5 sr / f0_floor + 0.5)`` the half window of
    the lowest f0, and f0 frame f has come (``env_frames_final``): the worst case over the batch, so ``push`` never reads the
    device.  The frames run through golf_spectral_envelope_stream_f32, the one-shot kernel at a position of the utterance.
    Samples before ``next_frame * hop - hwmax`` and f0 frames before ``next_frame`` are dropped (``env_keep_from``).

    ``latency = hwmax + 1`` samples beyond a frame's own time (512 at 24 kHz and n_fft 1024); behind an f0 stream the whole
    figure is ``max(latency, the f0 stream's latency)``.

    Inference only; one stream for the whole batch; ``push`` does no host-device synchronisation."""

    _module_type = SpectralEnvelopeAnalysis

    def __init__(self, module: SpectralEnvelopeAnalysis, batch_size: int):
        super().__init__(module, batch_size)
        self.hwmax = GF.spectral_envelope_hwmax(module.sample_rate, module.n_fft, module.f0_floor)
        self.span = 2 * self.hwmax + 1   # the longest window

    @property
    def latency(self) -> int:
        """The smallest number of samples beyond a frame's own time ``f * hop`` after which it can have been emitted."""
        return self.hwmax + 1

    def _total(self, final: bool) -> int:
        x, f0 = self._tracks
        return f0.end if final else env_frames_final(x.end, f0.end, self.hwmax, self.hop)

    def _keep(self):
        return env_keep_from(self._done, self.hwmax, self.hop)

    def _frames(self, x, f0, x_t0: int, f_first: int, f0_first: int, k: int, last: bool, full: bool):
        """``full``: ``(log_env, ceps)`` as ``analyse``; else what ``forward`` returns, one tensor."""
        m = self.module
        order = m.filter_order
        n_ceps = (m.n_fft // 2 + 1 if order is None else order + 1) if full else (None if order is None else order + 1)
        return GF.spectral_envelope_stream(x, f0, x_t0, f_first, f0_first, k, last, m.sample_rate, self.hop, m.n_fft, n_ceps,
                                           m.f0_floor, m.f0_ceil, m.unvoiced_f0, m.q1, m.eps, m.voiced_offset,
                                           return_log_env=full or order is None)

    def push(self, x=None, f0=None) -> AudioTensor:
        """The next block of the waveform and / or the next f0 frames -> the frames that became final, as ``forward``
        returns them."""
        return AudioTensor(self._run(x, f0, False, False), self.hop)

    def finish(self) -> AudioTensor:
        """The utterance has ended: the remaining frames; the stream starts a new utterance."""
        return AudioTensor(self._run(None, None, True, False), self.hop)

    def push_all(self, x=None, f0=None):
        """``push`` with the plain tensors of the module's ``analyse``: ``(log_env, ceps)``."""
        return self._run(x, f0, False, True)

    def finish_all(self):
        return self._run(None, None, True, True)


# ---- glottal-source analysis: the harmonic analysis of the residual, then the match against the table ------------------------
class GlottalSourceStream(_AudioF0Stream):
    """``glottal.GlottalSourceAnalysis`` block by block, for a live residual (a ``ResidualStream``) and its live f0.

    ``push(e=None, f0=None)`` takes the next (B, n) block of the residual and / or the next (B, k) f0 frames and returns
    ``w``, the ``table_select_weight`` of the frames that became final, an AudioTensor at ``hop_length``, possibly with zero
    frames; ``finish()`` ends the utterance (one frame per f0 frame received) and starts a new one; ``push_all`` /
    ``finish_all`` return the plain ``(w, theta, rho)`` of ``analyse``.  Everything pushed out plus ``finish()`` is
    ``torch.equal`` to ``analyse`` on the concatenated ``(e, f0)``, for any cuts and any interleaving.

    The bookkeeping is ``HarmonicNoiseStream``'s (``hna_frames_final``, ``hna_keep_from``) with the window arguments that
    ``analyse`` passes to ``functional.harmonic_analysis``: no noise bins, phases on, the module's ``unvoiced_window`` (4 hop).
    The frames that became final go through ``functional.harmonic_analysis_stream`` and then the module's ``match``, which
    is how ``analyse`` ends too: ``functional.glottal_match`` with the f0 values of exactly those frames, and
    ``unvoiced_weight`` for a frame without an estimate.  A push that completes no frame
    launches nothing.  ``latency`` is the audio side, as ``HarmonicNoiseStream.latency``; the frame also needs f0 frame
    ``f + 1``.

    Inference only; one stream for the whole batch; ``push`` does no host-device synchronisation."""

    _module_type = GlottalSourceAnalysis
    _audio = "e"

    def __init__(self, module: GlottalSourceAnalysis, batch_size: int):
        super().__init__(module, batch_size)
        self.unvoiced_window = module.unvoiced_window
        self.span = max(int(module.max_window), self.unvoiced_window)

    @property
    def latency(self) -> int:
        """The smallest number of samples beyond a frame's own time ``f * hop`` after which it can have been emitted: the
        residual's side.  The frame also needs f0 frame ``f + 1``."""
        return frame_reach(self.span, True)

    def _total(self, final: bool) -> int:
        x, f0 = self._tracks
        return f0.end if final else hna_frames_final(x.end, f0.end, self.span, self.hop)

    def _keep(self):
        return hna_keep_from(self._done, self.span, self.hop)

    def _frames(self, e, f0, x_t0: int, f_first: int, f0_first: int, k: int, last: bool, full: bool):
        m = self.module
        if k == 0:
            z = torch.empty(self.B, 0, dtype=torch.float32, device=self._device())
            return z, z.clone(), z.clone()
        amp, ph = GF.harmonic_analysis_stream(e, f0, x_t0, f_first, f0_first, k, last, m.sample_rate, self.hop,
                                              m.num_harmonics, None, m.periods, m.min_window, m.max_window,
                                              self.unvoiced_window, return_phases=True)
        return m.match(amp, ph, f0[:, f_first - f0_first:f_first - f0_first + k])

    def push(self, e=None, f0=None) -> AudioTensor:
        """The next block of the residual and / or the next f0 frames -> ``w`` of the frames that became final."""
        return AudioTensor(self._run(e, f0, False, True)[0], self.hop)

    def finish(self) -> AudioTensor:
        """The utterance has ended: the remaining frames; the stream starts a new utterance."""
        return AudioTensor(self._run(None, None, True, True)[0], self.hop)

    def push_all(self, e=None, f0=None):
        """``push`` with the plain tensors of the module's ``analyse``: ``(w, theta, rho)``."""
        return self._run(e, f0, False, True)

    def finish_all(self):
        return self._run(None, None, True, True)


# ---- the residual: samples out, from samples and frame-rate filter parameters ------------------------------------------------
def res_samples_final(pushed: int, frames_received: int, hop: int) -> int:
    """Samples of a ``ResidualStream``, counted from 0, that are final after ``pushed`` samples and ``frames_received``
    frames of ``(gain, a)``: sample t is final once it has come and so has frame ``t // hop + 1``, the far end of its
    interpolation.  (The last sample of an utterance, which the clamp ``f <= F - 2`` serves, is known only at ``finish()``.)"""
    return min(pushed, max(frames_received - 1, 0) * hop)


def res_samples_finish(pushed: int, frames_received: int, hop: int) -> int:
    """Samples of the whole utterance: ``min(T, (F - 1) hop + 1)``, 0 without a frame."""
    return min(pushed, (frames_received - 1) * hop + 1) if frames_received >= 1 else 0


def res_keep_from(emitted: int, frames_received: int, order: int, hop: int):
    """``(sample, frame)`` from which a ``ResidualStream`` that has emitted ``emitted`` samples keeps its inputs: the first
    tap of the next sample, and that sample's frame ``emitted // hop`` -- but never above frame ``frames_received - 2``,
    which the next sample reads through the clamp if the utterance ends with the frames received so far."""
    return max(emitted - order, 0), max(min(emitted // hop, frames_received - 2), 0)


class ResidualStream(_Stream):
    """``functional.ltv_residual`` (``GlottalSourceAnalysis.residual_fused``) block by block: live audio and the live
    ``(gain, a)`` of an ``LPCAnalysisStream`` on the same audio -> the excitation estimate that a ``GlottalSourceStream``
    reads.

    ``push(x=None, gain=None, a=None)`` takes the next (B, n) block of the waveform and / or the next frames ``gain`` (B, k)
    and ``a`` (B, k, lpc_order), which come together (tensors, or AudioTensors at ``hop_length``), and returns ``e`` (B, m),
    the samples that became final, possibly none.  ``finish()`` ends the utterance -- F = the frames received, T = the samples
    received, ``T' = min(T, (F - 1) hop + 1)`` samples in all, none when F = 0 -- returns the rest and starts a new utterance.
    ``push_all`` / ``finish_all`` are the same calls (the result is a plain tensor either way).  Everything pushed out plus
    ``finish()`` is ``torch.equal`` to ``functional.ltv_residual`` on the concatenated inputs, for any cuts and any
    interleaving.

    Sample t is final once it has come and so has frame ``t // hop + 1`` (``res_samples_final``); sample ``(F - 1) hop``, which
    the one-shot interpolates through the clamp ``f <= F - 2``, comes out at ``finish()`` only.  The samples run through
    golf_ltv_residual_stream_f32, the one-shot kernel at a position of the utterance.  Samples before ``emitted - lpc_order``
    and frames before ``min(emitted // hop, frames received - 2)`` are dropped (``res_keep_from``); whichever input runs
    ahead is held until the other catches up.

    ``latency``: sample t needs frame ``t // hop + 1``, whose own time is at most ``hop`` samples after t; with frames that
    arrive d samples after their own time, ``e[t]`` can have been emitted ``hop + d`` samples after t.  ``latency`` is the
    stream's own part, ``hop``; behind a centred ``LPCAnalysisStream`` d is half its window, 240 + 480 = 720 samples at the
    recipe (hop 240, window 960).

    Inference only; one stream for the whole batch; ``push`` does no host-device synchronisation."""

    def __init__(self, hop_length: int, lpc_order: int, batch_size: int):
        super().__init__(batch_size, hop_length, 3)   # the tracks: x, and gain and a, which move together
        self.order = int(lpc_order)
        if not 1 <= self.order <= GF.RES_MAX_ORDER:
            raise _lib.GolfError(f"{self._who}: lpc_order={self.order} must be 1..{GF.RES_MAX_ORDER}")

    frames_received = property(lambda self: self._tracks[1].end, doc="Frames of (gain, a) of this utterance so far.")
    emitted = property(lambda self: self._done, doc="Samples emitted so far.")

    @property
    def latency(self) -> int:
        """The stream's own part of the delay of ``e[t]`` behind sample t: ``hop`` samples, to the own time of frame
        ``t // hop + 1``; the delay d of the frames behind their own time adds to it (class docstring)."""
        return self.hop

    def _require_device(self, *tensors) -> None:
        _lib.require_device(*tensors)

    def _samples(self, x, gain, a, x_t0: int, fr_first: int, t_first: int, n: int, last: bool):
        """Samples ``t_first .. t_first + n - 1`` from the buffers, which start at sample ``x_t0`` and frame ``fr_first``."""
        if n == 0:
            return torch.empty(self.B, 0, dtype=torch.float32, device=self._device())
        return GF.ltv_residual_stream(x, gain, a, x_t0, fr_first, t_first, n, last, self.hop)

    def _total(self, final: bool) -> int:
        return (res_samples_finish if final else res_samples_final)(self._tracks[0].end, self._tracks[1].end, self.hop)

    def _keep(self):
        x_from, f_from = res_keep_from(self._done, self._tracks[1].end, self.order, self.hop)
        return x_from, f_from, f_from

    def _compute(self, n: int, final: bool):
        x, gain, a = self._tracks
        return self._samples(x.data, gain.data, a.data, x.start, gain.start, self._done, n, final)

    def _run(self, x, gain, a, final: bool):
        if (gain is None) != (a is None):
            raise ValueError(f"{self._who}.push: gain and a come together")
        x = None if x is None else self._check_block(x, "x", 1)   # every block is checked before any device is looked at
        if gain is not None:
            gain, a = self._check_block(gain, "gain", self.hop), self._check_block(a, "a", self.hop, 3)
            if a.shape[1] != gain.shape[1] or a.shape[2] != self.order:
                raise ValueError(f"{self._who}.push: a of shape {tuple(a.shape)} beside gain {tuple(gain.shape)}; the "
                                 f"stream has lpc_order={self.order}")
        self._require_device(x, gain, a)
        return self._advance((x, gain, a), final)

    def push(self, x=None, gain=None, a=None) -> torch.Tensor:
        """The next block of the waveform and / or the next frames of ``(gain, a)`` -> the samples of ``e`` that became
        final."""
        return self._run(x, gain, a, False)

    def finish(self) -> torch.Tensor:
        """The utterance has ended: the remaining samples; the stream starts a new utterance."""
        return self._run(None, None, None, True)

    push_all, finish_all = push, finish


def open_analysis_stream(module, batch_size: int, **kw):
    """The stream of an analysis module: ``F0TrackerStream`` (``lag=``), ``F0Stream``, ``LPCAnalysisStream``
    (``return_rc=``), ``SourceFilterLPCStream`` (``return_rc=``, ``return_source=``), ``HarmonicNoiseStream``,
    ``SpectralEnvelopeStream`` or ``GlottalSourceStream``.  (``ResidualStream`` has no module: it is opened with the hop and
    the order.)"""
    if isinstance(module, SpectralEnvelopeAnalysis):
        return SpectralEnvelopeStream(module, batch_size, **kw)
    if isinstance(module, GlottalSourceAnalysis):
        return GlottalSourceStream(module, batch_size, **kw)
    if isinstance(module, HarmonicNoiseAnalysis):
        return HarmonicNoiseStream(module, batch_size, **kw)
    if isinstance(module, F0Tracker):
        return F0TrackerStream(module, batch_size, **kw)
    if isinstance(module, F0Analysis):
        return F0Stream(module, batch_size, **kw)
    if isinstance(module, LPCAnalysis):
        return LPCAnalysisStream(module, batch_size, **kw)
    if isinstance(module, SourceFilterLPCAnalysis):
        return SourceFilterLPCStream(module, batch_size, **kw)
    raise TypeError(f"open_analysis_stream: no analysis stream for {type(module).__name__}")
