"""Block-by-block analysis: the streaming counterparts of ``f0.F0Analysis``, ``f0.F0Tracker`` and ``lpc.LPCAnalysis``, for a
live waveform that feeds a decoder stream (``stream.DecoderStream`` and its siblings take exactly these tracks).

The protocol is the decoder streams': ``push(x)`` takes the next (B, n) block of the waveform, any n >= 0, and returns the
frames that became final, in the types the module's ``forward`` returns (possibly with zero frames); ``finish()`` ends the
utterance, returns the rest and leaves the stream ready for a new utterance.  Everything pushed out plus ``finish()`` is
``torch.equal`` to the one-shot module on the concatenated input, whatever the cuts.

YIN frames and LPC frames are frame-local: a frame is final once its last sample has come, and the one-shot kernels run
``centred=False, n_frames=`` on the buffered samples that the open frames still need -- a frame's arithmetic does not depend
on where it sits in the row, which is why the result is exact.  Zeros stand before sample 0 and after the end, as the
definitions say.  The tracker is not frame-local: its candidates are, and the path through them is decided ``lag`` frames
late by golf_f0_viterbi_stream_f32 (csrc/f0_viterbi_stream.hip), whose costs are carried from push to push.

Inference only; one stream for the whole batch; ``push`` does no host-device synchronisation.
"""
from __future__ import annotations

import torch

from . import _lib
from . import functional as GF
from .audiotensor import AudioTensor
from .f0 import F0Analysis, F0Tracker
from .lpc import LPCAnalysis

__all__ = ["F0Stream", "F0TrackerStream", "LPCAnalysisStream", "open_analysis_stream", "frames_open", "frames_final",
           "frame_reach"]


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


class _FrameStream:
    """The protocol and the sample buffer the three streams share.  A subclass names its frame (``span``, ``hop``,
    ``centred``) and implements ``_frames(x, k)``: the one-shot call for the first k frames of x with ``centred=False``."""

    def __init__(self, module, batch_size: int, span: int):
        if int(batch_size) < 1:
            raise ValueError(f"{self._who}: batch_size={batch_size}")
        self.module, self.B = module, int(batch_size)
        self.span, self.hop, self.centred = int(span), int(module.hop_length), bool(module.centred)
        if self.hop < 1:
            raise _lib.GolfError(f"{self._who}: hop={self.hop} must be >= 1")
        self._origin = -(self.span // 2) if self.centred else 0
        self._buf = None     # (B, m) fp32: samples [_buf0, _buf0 + m) with zeros before sample 0
        self._reset()

    @property
    def _who(self) -> str:
        return type(self).__name__

    def _reset(self) -> None:
        self.pushed = 0      # samples of this utterance so far
        self.framed = 0      # frames handed to the kernels so far
        self._buf0 = self._origin
        if self._buf is not None:
            self._buf = self._buf.new_zeros(self.B, -self._origin)

    @property
    def latency(self) -> int:
        """The smallest number of samples beyond a frame's own time ``f * hop`` after which it has been emitted."""
        return frame_reach(self.span, self.centred)

    def _take(self, x) -> torch.Tensor:
        if isinstance(x, AudioTensor):
            assert x.hop_length == 1, f"the waveform must be at hop 1 (got {x.hop_length})"
            x = x.as_tensor()
        if x.dim() != 2 or x.shape[0] != self.B:
            raise ValueError(f"{self._who}.push: x of shape {tuple(x.shape)}; the stream has B={self.B}")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError(f"{self._who}: an input that requires grad (streaming is inference only) is not supported")
        if torch.is_autocast_enabled() and x.is_floating_point():   # as the one-shot functions: fp16 / bf16 become fp32
            x = x.float()
        _lib.require_device(x)
        return x.detach()

    def _append(self, x: torch.Tensor) -> None:
        if self._buf is None:
            self._buf = x.new_zeros(self.B, -self._origin)
        keep = x[:, min(max(self._buf0 - self.pushed, 0), x.shape[1]):]   # hop > span: samples between frames are dropped
        if keep.shape[1]:
            self._buf = torch.cat([self._buf, keep], 1) if self._buf.shape[1] else keep
        self.pushed += x.shape[1]

    def _advance(self, final: bool):
        """The frames that became final, through the one-shot kernels; the samples no open frame needs are dropped."""
        total = frames_final(self.pushed, self.span, self.hop, self.centred) if final else \
            frames_open(self.pushed, self.span, self.hop, self.centred)
        k = total - self.framed
        out = None
        if k > 0:
            start = self._origin + self.framed * self.hop   # >= _buf0: nothing before it was kept
            x = self._buf[:, max(start - self._buf0, 0):] if start < self._buf0 + self._buf.shape[1] else None
            if x is None or x.shape[1] == 0:
                x = self._buf.new_zeros(self.B, 1)          # the frames read only the zeros after the end
            out = self._frames(x, k)
            self.framed = total
        nxt = self._origin + self.framed * self.hop
        if nxt > self._buf0:
            self._buf = self._buf[:, min(nxt - self._buf0, self._buf.shape[1]):]
            self._buf0 = nxt
        return k, out

    def _device(self):
        return self._buf.device if self._buf is not None else torch.device("cuda")

    def _run(self, x, final: bool):
        if x is not None:
            x = self._take(x)
        with torch.no_grad():
            if x is not None:
                self._append(x)
            elif self._buf is None:
                self._buf = torch.zeros(self.B, -self._origin, device=self._device())
            out = self._emit(*self._advance(final), final)
            if final:
                self._reset()
            return out


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
        return GF.f0_viterbi_stream(period, ap, self._carry, self.framed - k, self.lag, m.sample_rate, float(m.tau_min),
                                    m.unvoiced_cost, m.lag_cost, m.jump_cost, m.switch_cost, flush=final, return_state=True)


class LPCAnalysisStream(_FrameStream):
    """``LPCAnalysis`` block by block: ``push`` / ``finish`` give ``(gain, a)`` as ``forward`` does -- the
    ``end_filter_params`` of a decoder stream -- and with ``return_rc=True`` ``(gain, a, rc)``; ``push_all`` / ``finish_all``
    give the plain tensors of ``analyse``.  A frame is emitted once its last sample has been pushed."""

    def __init__(self, module: LPCAnalysis, batch_size: int, return_rc: bool = False):
        if not isinstance(module, LPCAnalysis):
            raise TypeError(f"LPCAnalysisStream: an LPCAnalysis is needed (got {type(module).__name__})")
        super().__init__(module, batch_size, module.window_length)
        self.return_rc = bool(return_rc)

    def _frames(self, x, k):
        m = self.module
        return GF.lpc_analysis(x, m._window, self.hop, m.lpc_order, centred=False, n_frames=k, return_rc=self.return_rc)

    def _emit(self, k, out, final):
        if k > 0:
            return out
        dev, M = self._device(), self.module.lpc_order
        gain = torch.empty(self.B, 0, dtype=torch.float32, device=dev)
        a = torch.empty(self.B, 0, M, dtype=torch.float32, device=dev)
        return (gain, a, a.clone()) if self.return_rc else (gain, a)

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


def open_analysis_stream(module, batch_size: int, **kw):
    """The stream of an analysis module: ``F0TrackerStream`` (``lag=``), ``F0Stream`` or ``LPCAnalysisStream``
    (``return_rc=``)."""
    if isinstance(module, F0Tracker):
        return F0TrackerStream(module, batch_size, **kw)
    if isinstance(module, F0Analysis):
        return F0Stream(module, batch_size, **kw)
    if isinstance(module, LPCAnalysis):
        return LPCAnalysisStream(module, batch_size, **kw)
    raise TypeError(f"open_analysis_stream: no analysis stream for {type(module).__name__}")
