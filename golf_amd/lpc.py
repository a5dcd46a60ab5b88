"""Frame-wise LPC synthesisers of the reference's models/lpc.py, MI355X-native.

``BatchSecondOrderLPCSynth`` (reference models/lpc.py:94-131) is the reference's statement of the *cascaded-biquad*
all-pole filter: every frame runs through K second-order sections.  Here the cascade is a systolic pipeline across
the lanes of a DPP row (golf_biquad_frames_ola_fwd_f32, csrc/lpc_ff.hip), and so is its backward
(golf_biquad_frames_ola_bwd_f32: the adjoint of a cascade is the reversed cascade on the reversed signal), so the module is
differentiable w.r.t. the excitation, the gains and the section coefficients like the reference's (autograd through its K
lfilter calls, models/lpc.py:115-118).
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from . import functional as GF
from .audiotensor import AudioTensor
from .utils import get_window_fn

__all__ = ["BatchSecondOrderLPCSynth", "LPCAnalysis", "SourceFilterLPCAnalysis"]


class LPCAnalysis(nn.Module):
    """Frame-wise LPC analysis by the autocorrelation method: a waveform -> ``(gain, a)`` at hop ``hop_length``, on the
    device and differentiable w.r.t. the waveform (golf_lpc_analysis_{fwd,bwd}_f32, fp64 lags and recursion).  The
    reference has no such module; its output is the ``end_filter_params`` tuple that ``LTVMinimumPhaseFilterPrecise`` and
    ``LTVMinimumPhaseFilter`` take in ``forward`` and in ``reverse``: analysis / resynthesis, residual extraction, targets
    for the encoder head (``logits``), LPC-domain losses on synthesised audio.

    ``centred=True`` puts frame f around sample ``f * hop_length`` (the filters' frame grid, ``T // hop_length + 1``
    frames); ``centred=False`` starts it there.  ``gain = sqrt(prediction error / sum(window**2))``: a unit-variance
    excitation through ``a`` reproduces the frame's level."""

    def __init__(self, lpc_order: int, hop_length: int, window_length: int = None, window: str = "hann",
                 centred: bool = True):
        super().__init__()
        self.lpc_order = lpc_order
        self.hop_length = hop_length
        self.window_length = hop_length * 4 if window_length is None else window_length
        self.centred = centred
        self.register_buffer("_window", get_window_fn(window)(self.window_length).float(), persistent=False)

    def analyse(self, x, return_rc: bool = False):
        """Plain tensors: ``(gain (B, F), a (B, F, M))`` or ``(gain, a, rc)``."""
        if isinstance(x, AudioTensor):
            assert x.hop_length == 1, f"the waveform must be at hop 1 (got {x.hop_length})"
            x = x.as_tensor()
        assert x.ndim == 2, x.shape
        return GF.lpc_analysis(x, self._window, self.hop_length, self.lpc_order, centred=self.centred, return_rc=return_rc)

    def forward(self, x):
        gain, a = self.analyse(x)
        return AudioTensor(gain, self.hop_length), AudioTensor(a, self.hop_length)

    @staticmethod
    def to_logits(gain: Tensor, rc: Tensor, max_abs_value: float = 1.0):
        """``(log_gain (B, F, 1), lpc_logits (B, F, M))``: the inverse of the ``rc2lpc`` control transform
        ``(exp(log_gain), rc2lpc(tanh(lpc_logits) * max_abs_value))``."""
        lim = 1.0 - 1e-6
        return torch.log(gain).unsqueeze(-1), torch.atanh(torch.clamp(rc / max_abs_value, -lim, lim))

    def logits(self, x, max_abs_value: float = 1.0):
        """Targets for an encoder head that drives ``LTVMinimumPhaseFilterPrecise(lpc_parameterisation="rc2lpc")``."""
        gain, _, rc = self.analyse(x, return_rc=True)
        return self.to_logits(gain, rc, max_abs_value)


class SourceFilterLPCAnalysis(nn.Module):
    """Source-compensated LPC analysis: a waveform -> ``(gain, a)`` at hop ``hop_length`` with the glottal source's spectral
    tilt estimated beside the vocal tract and kept out of ``a`` (golf_lpc_source_filter_f32: iterative adaptive inverse
    filtering on the frame's lags, fp64).  ``LPCAnalysis`` fits one all-pole model to the whole spectrum; the GOLF decoders
    keep the tilt in the wavetable and expect ``a`` to be the tract alone, which is what ``GlottalSourceAnalysis`` needs of
    its residual.  Same frames and the same ``end_filter_params`` tuple as ``LPCAnalysis``; ``gain`` is the level of the
    audio through ``a``'s inverse alone.  ``source_order`` and ``iterations`` size the source model and the rounds of tract
    against source; ``preemphasis`` fixes the first source polynomial to ``1 - preemphasis z^-1`` instead of fitting it to
    the frame.  Inference only: the outputs never require grad."""

    def __init__(self, lpc_order: int, hop_length: int, window_length: int = None, window: str = "hann",
                 centred: bool = True, source_order: int = 4, iterations: int = 2, preemphasis: float = None):
        super().__init__()
        self.lpc_order = lpc_order
        self.hop_length = hop_length
        self.window_length = hop_length * 4 if window_length is None else window_length
        self.centred = centred
        self.source_order = source_order
        self.iterations = iterations
        self.preemphasis = preemphasis
        self.register_buffer("_window", get_window_fn(window)(self.window_length).float(), persistent=False)

    def analyse(self, x, return_rc: bool = False, return_source: bool = False):
        """Plain tensors: ``(gain (B, F), a (B, F, M))``, then ``rc`` and ``source (B, F, Q)`` as asked for."""
        if isinstance(x, AudioTensor):
            assert x.hop_length == 1, f"the waveform must be at hop 1 (got {x.hop_length})"
            x = x.as_tensor()
        assert x.ndim == 2, x.shape
        return GF.source_filter_lpc(x, self._window, self.hop_length, self.lpc_order, self.source_order, self.iterations,
                                    self.preemphasis, centred=self.centred, return_rc=return_rc,
                                    return_source=return_source)

    def forward(self, x):
        gain, a = self.analyse(x)
        return AudioTensor(gain, self.hop_length), AudioTensor(a, self.hop_length)

    def logits(self, x, max_abs_value: float = 1.0):
        """``LPCAnalysis.to_logits`` of this analysis: targets for an ``rc2lpc`` encoder head."""
        gain, _, rc = self.analyse(x, return_rc=True)
        return LPCAnalysis.to_logits(gain, rc, max_abs_value)


class BatchSecondOrderLPCSynth(nn.Module):
    def __init__(self, hop_length: int, window_size: int = None, window: str = "hann"):
        super().__init__()
        self.hop_length = hop_length
        self.window_size = hop_length * 4 if window_size is None else window_size
        self.padding = (self.window_size - self.hop_length) // 2
        # the reference keeps diag(window) as a (W,1,W) conv kernel `_kernel`; only its diagonal is ever used
        self.register_buffer("_window", get_window_fn(window)(self.window_size).float(), persistent=False)

    def forward(self, ex: Tensor, gain: Tensor, biquads: Tensor) -> Tensor:
        assert ex.ndim == 2
        assert gain.ndim == 2
        assert biquads.ndim == 4 and biquads.shape[-1] == 3
        return GF.biquad_frames_ola(ex, gain, biquads, self._window, self.hop_length, pad=self.padding, frame_gain=True)
