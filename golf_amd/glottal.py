"""Glottal-source analysis: the counterpart of the glottal-flow wavetable's control, as ``lpc.LPCAnalysis`` is of the end
filter's, ``f0.F0Analysis`` of the f0, ``hna.HarmonicNoiseAnalysis`` of the harmonic-plus-noise decoders' and
``envelope.SpectralEnvelopeAnalysis`` of the cepstral filter's.

The GOLF decoder's source (``synth.IndexedGlottalFlowTable`` and its subclasses) takes ``table_select_weight`` (B, F) in
[0, 1], the position on the table's R_d grid: which glottal pulse.  The reference has only a trained encoder to produce it.
``GlottalSourceAnalysis`` measures it on a recording: the audio through the inverse of its all-pole filter
(``functional.ltv_inverse``) and divided by the gain is the decoder's excitation estimate; its harmonics at each frame centre
(``functional.harmonic_analysis``) are matched against every table row at every phase shift by one HIP kernel
(golf_glottal_match_f32, csrc/glottal_match.hip; the definition is in include/golf_amd.h).
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["GlottalSourceAnalysis"]


class GlottalSourceAnalysis(nn.Module):
    """(residual, f0) -> ``table_select_weight`` (B, F) at hop ``hop_length``, on the device (no parameters, no gradient).
    ``table`` is a ``synth.GlottalFlowTable`` (any subclass; it becomes a submodule, and a trainable table is followed) or a
    (K, L) tensor.  Frame f is centred on sample ``f * hop_length``, the decoders' frame grid; ``f0`` is in Hz with 0 for
    unvoiced frames, as ``F0Analysis`` gives it.  ``num_harmonics`` harmonics are matched at ``n_phi`` phase shifts;
    ``unvoiced_weight`` fills the frames that have no estimate; ``periods``, ``min_window`` and ``max_window`` are the
    window arguments of ``functional.harmonic_analysis``."""

    def __init__(self, table, sample_rate: float, hop_length: int, num_harmonics: int = 64, n_phi: int = 256,
                 unvoiced_weight: float = 0.5, periods: int = 4, min_window: int = None, max_window: int = 2048):
        super().__init__()
        if isinstance(table, nn.Module):
            if not isinstance(getattr(table, "table", None), torch.Tensor):
                raise TypeError("table must be a GlottalFlowTable or a (K, L) tensor")
            self.source = table
        elif isinstance(table, torch.Tensor):
            self.source = None
            self.register_buffer("table", table.detach().clone(), persistent=False)
        else:
            raise TypeError("table must be a GlottalFlowTable or a (K, L) tensor")
        self.sample_rate, self.hop_length, self.num_harmonics, self.n_phi = sample_rate, hop_length, num_harmonics, n_phi
        self.unvoiced_weight, self.periods, self.max_window = unvoiced_weight, periods, max_window
        self.min_window = 2 * hop_length if min_window is None else min_window
        GF.glottal_plan(self._table(), num_harmonics)   # refuses a table or a harmonic count the kernel does not take
        self._plan_key = None
        for name in ("_plan_spectrum", "_plan_norms", "_plan_cross"):
            self.register_buffer(name, None, persistent=False)

    def _table(self) -> torch.Tensor:
        return self.table if self.source is None else self.source.table

    def plan(self) -> GF.GlottalPlan:
        """The table's ``functional.glottal_plan``, kept in non-persistent buffers and rebuilt when the table's storage, its
        version counter (an optimiser step on a trainable table, any other in-place change) or its device has changed."""
        t = self._table()
        key = (t.data_ptr(), t._version, t.device, int(self.num_harmonics))
        if self._plan_key != key or self._plan_spectrum is None or self._plan_spectrum.device != t.device:
            p = GF.glottal_plan(t, self.num_harmonics)
            self._plan_spectrum, self._plan_norms, self._plan_cross = p.spectrum, p.norms, p.cross
            self._plan_key = key
        return GF.GlottalPlan(self._plan_spectrum, self._plan_norms, self._plan_cross)

    def _plain(self, t, hop, what):
        if isinstance(t, AudioTensor):
            assert t.hop_length == hop, f"{what} must be at hop {hop} (got {t.hop_length})"
            return t.as_tensor()
        return t

    def residual(self, x, gain, a) -> torch.Tensor:
        """The decoder's excitation estimate (B, T'): ``functional.ltv_inverse(x, a, hop_length)`` divided by the gain
        upsampled linearly as the end filter upsamples it (``gain`` (B, F), ``a`` (B, F, M), as ``LPCAnalysis`` gives
        them); ``T' = min(T, (F - 1) hop_length + 1)``."""
        x = self._plain(x, 1, "the waveform")
        gain, a = self._plain(gain, self.hop_length, "gain"), self._plain(a, self.hop_length, "a")
        e = GF.ltv_inverse(x, a, self.hop_length)
        return e / GF.linear_upsample(gain, self.hop_length)[:, :e.shape[1]]

    def residual_fused(self, x, gain, a) -> torch.Tensor:
        """``residual`` in one launch (``functional.ltv_residual``, golf_ltv_residual_f32): the same inverse filter, bit for
        bit, divided by the gain interpolated as ``fmaf(w, gain[f+1] - gain[f], gain[f])``, ``w = (t - f hop) / hop``.  It
        differs from ``residual`` only in how the gain is interpolated (there torch forms the weight as ``fl(1 / hop) t``,
        whose error grows with t); every sample is a function of its position alone, so this is the definition that
        ``analysis_stream.ResidualStream`` is exact against.  No gradient."""
        x = self._plain(x, 1, "the waveform")
        gain, a = self._plain(gain, self.hop_length, "gain"), self._plain(a, self.hop_length, "a")
        return GF.ltv_residual(x, gain, a, self.hop_length)

    def analyse(self, e, f0):
        """Plain tensors ``(w, theta, rho)``, (B, F) each: the table position with ``unvoiced_weight`` where there is no
        estimate, the table phase at the frame's centre in cycles and the fit in [-1, 1] (0 where there is no estimate)."""
        e, f0 = self._plain(e, 1, "the residual"), self._plain(f0, self.hop_length, "f0")
        assert e.ndim == 2, e.shape
        assert f0.ndim == 2, f0.shape
        amp, ph = GF.harmonic_analysis(e, f0, self.sample_rate, self.hop_length, self.num_harmonics, None, self.periods,
                                       self.min_window, self.max_window, self.unvoiced_window, return_phases=True)
        return self.match(amp, ph, f0)

    @property
    def unvoiced_window(self) -> int:
        """The window of an unvoiced frame: what ``functional.harmonic_analysis`` takes when it is left out."""
        return 4 * int(self.hop_length)

    def match(self, amp, ph, f0):
        """``(w, theta, rho)`` of frames whose harmonics ``(amp, ph)`` the harmonic analysis of the residual gave and whose
        f0 is ``f0``: ``functional.glottal_match`` against the table, then ``unvoiced_weight`` where there is no estimate.
        ``analyse`` and ``analysis_stream.GlottalSourceStream`` both end with it."""
        w, theta, rho = GF.glottal_match(amp, ph, f0, self.plan(), self.sample_rate, self.n_phi)
        return torch.nan_to_num_(w, nan=float(self.unvoiced_weight)), theta, rho

    def forward(self, e, f0) -> AudioTensor:
        return AudioTensor(self.analyse(e, f0)[0], self.hop_length)

    def logits(self, e, f0) -> torch.Tensor:
        """``logit(clamp(w, 1e-6, 1 - 1e-6))`` (B, F): the target of the oscillator's ``ctrl`` (sigmoid) head."""
        return torch.logit(self.analyse(e, f0)[0].clamp_(1e-6, 1 - 1e-6))

    def synthesise(self, f0, w, gain, a, log_mag=None, noise=None, window: str = "hanning", oversampling: int = 4) -> AudioTensor:
        """The GOLF-ss copy-synthesis of analysed controls on the package's own modules: the table oscillator on
        ``f0 / sample_rate`` and ``w`` (``source`` itself when it is an ``IndexedGlottalFlowTable``, else
        ``functional.glottal_osc`` on the table at ``oversampling``), plus, with ``log_mag`` (from
        ``HarmonicNoiseAnalysis``), ``LTVZeroPhaseFIRFilter(window)`` on ``noise`` (N(0, 1) drawn on the device when None),
        through ``LTVMinimumPhaseFilterPrecise`` with ``gain`` and ``a``.  The pulses start at phase 0: ``theta`` is not used.
        ``f0`` must be positive in every frame (fill unvoiced frames as the decoder's f0 track is filled)."""
        from .filters import LTVMinimumPhaseFilterPrecise, LTVZeroPhaseFIRFilter
        from .synth import Decimate, IndexedGlottalFlowTable

        f0, w, gain, a, log_mag = (self._plain(t, self.hop_length, "controls") for t in (f0, w, gain, a, log_mag))
        phase = AudioTensor(f0 / self.sample_rate, self.hop_length)
        if isinstance(self.source, IndexedGlottalFlowTable):
            ex = self.source(phase, AudioTensor(w, self.hop_length)).as_tensor()
        else:
            taps = Decimate(oversampling).taps.to(f0.device) if oversampling > 1 else None
            ex = GF.glottal_osc(phase.as_tensor(), w, self._table().detach(), taps, phase_hop=self.hop_length,
                                w_hop=self.hop_length, oversampling=oversampling)
        if log_mag is not None:
            if noise is None:
                noise = torch.randn_like(ex)
            elif isinstance(noise, AudioTensor):
                assert noise.hop_length == 1, f"the noise must be at hop 1 (got {noise.hop_length})"
                noise = noise.as_tensor()
            v = LTVZeroPhaseFIRFilter(window)(AudioTensor(noise), AudioTensor(log_mag, self.hop_length)).as_tensor()
            n = min(ex.shape[1], v.shape[1])
            ex = ex[:, :n] + v[:, :n]
        end = LTVMinimumPhaseFilterPrecise()
        return end(AudioTensor(ex), AudioTensor(gain, self.hop_length), AudioTensor(a, self.hop_length))
