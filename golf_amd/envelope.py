"""Spectral-envelope analysis: the counterpart of the NHV decoder's harmonic-filter control, as ``lpc.LPCAnalysis`` is of the
end filter's, ``f0.F0Analysis`` of the f0 and ``hna.HarmonicNoiseAnalysis`` of the harmonic-plus-noise decoders'.

The cepstral harmonic filter (``filters.LTVCepFilter``, fed by ``synth.AdditivePulseTrain`` in the NHV decoder) takes ``ceps``
rows (B, F, filter_order + 1) and ``functional.stft_filter_frames`` takes response rows (B, F, n_fft/2 + 1); the reference
has only a trained encoder to produce them.  ``SpectralEnvelopeAnalysis`` measures both on a recording with a known f0 track:
a pitch-adaptive envelope estimator of the CheapTrick kind (an f0-sized window, a power spectrum, smoothing over 2 f0 / 3,
cepstral liftering), one HIP kernel (golf_spectral_envelope_f32, csrc/spec_envelope.hip; the definition is in
include/golf_amd.h).  The WORLD decoder's ``mel_sp`` is not produced: ``DiffWorldSPFilter`` maps it through the rectified
pseudo-inverse of a mel filterbank, which no choice of ``mel_sp`` brings back to a given envelope;
``log_env`` is what a WORLD-style user can take instead.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["SpectralEnvelopeAnalysis"]


class SpectralEnvelopeAnalysis(nn.Module):
    """(waveform, f0) -> ``ceps`` (B, F, filter_order + 1) at hop ``hop_length`` when ``filter_order`` is given, else
    ``log_env`` (B, F, n_fft/2 + 1), on the device (no parameters, no buffers, no gradient).  Frame f is centred on sample
    ``f * hop_length``, the decoders' frame grid; ``f0`` is in Hz with 0 for unvoiced frames, as ``F0Analysis`` gives it.
    The remaining arguments are those of ``functional.spectral_envelope``."""

    def __init__(self, sample_rate: float, hop_length: int, n_fft: int = 1024, filter_order: int = None,
                 f0_floor: float = None, f0_ceil: float = None, unvoiced_f0: float = 500.0, q1: float = -0.15,
                 eps: float = 1e-12, voiced_offset: float = GF.ENV_VOICED_OFFSET):
        super().__init__()
        self.sample_rate, self.hop_length, self.n_fft, self.filter_order = sample_rate, hop_length, n_fft, filter_order
        lo, hi = GF.spectral_envelope_defaults(float(sample_rate), int(n_fft))
        self.f0_floor, self.f0_ceil = lo if f0_floor is None else f0_floor, hi if f0_ceil is None else f0_ceil
        self.unvoiced_f0, self.q1, self.eps, self.voiced_offset = unvoiced_f0, q1, eps, voiced_offset

    def _plain(self, t, hop, what):
        if isinstance(t, AudioTensor):
            assert t.hop_length == hop, f"{what} must be at hop {hop} (got {t.hop_length})"
            return t.as_tensor()
        return t

    def _run(self, x, f0, n_ceps, return_log_env: bool):
        x, f0 = self._plain(x, 1, "the waveform"), self._plain(f0, self.hop_length, "f0")
        assert x.ndim == 2, x.shape
        assert f0.ndim == 2, f0.shape
        return GF.spectral_envelope(x, f0, self.sample_rate, self.hop_length, self.n_fft, n_ceps, self.f0_floor, self.f0_ceil,
                                    self.unvoiced_f0, self.q1, self.eps, self.voiced_offset, return_log_env=return_log_env)

    def analyse(self, x, f0):
        """Plain tensors ``(log_env, ceps)``: the log magnitude envelope (B, F, n_fft/2 + 1) and the cepstrum (B, F,
        filter_order + 1; all n_fft/2 + 1 coefficients when ``filter_order`` is None)."""
        return self._run(x, f0, self.n_fft // 2 + 1 if self.filter_order is None else self.filter_order + 1, True)

    def response_rows(self, x, f0) -> torch.Tensor:
        """``exp(log_env)`` (B, F, n_fft/2 + 1): the zero-phase response rows ``functional.stft_filter_frames`` takes."""
        return torch.exp_(self._run(x, f0, None, True))

    def forward(self, x, f0) -> AudioTensor:
        if self.filter_order is None:
            return AudioTensor(self._run(x, f0, None, True), self.hop_length)
        return AudioTensor(self._run(x, f0, self.filter_order + 1, False), self.hop_length)

    def synthesise(self, f0, ceps, log_mag=None, noise=None, window: str = "hanning", phase: str = "min",
                   num_harmonics: int = 155) -> AudioTensor:
        """The NHV copy-synthesis of analysed controls on the package's own modules: ``AdditivePulseTrain(num_harmonics)`` on
        ``f0 / sample_rate`` into ``LTVCepFilter(ceps.shape[-1] - 1, n_fft, window, hop_length, phase)``, plus, with
        ``log_mag`` (from ``HarmonicNoiseAnalysis``), ``LTVZeroPhaseFIRFilter(window)`` on ``noise`` (N(0, 1) drawn on the
        device when None), truncated to the shorter of the two.  ``f0`` must be positive in every frame (fill unvoiced
        frames as the decoder's f0 track is filled): the pulse train's equal-energy factor is ``sqrt(2 f0 / sr)``."""
        from .filters import LTVCepFilter, LTVZeroPhaseFIRFilter
        from .synth import AdditivePulseTrain

        f0, ceps, log_mag = (self._plain(t, self.hop_length, "controls") for t in (f0, ceps, log_mag))
        phase_track = AudioTensor(f0 / self.sample_rate, self.hop_length)
        pulses = AdditivePulseTrain(num_harmonics)(phase_track)
        cep_filter = LTVCepFilter(ceps.shape[-1] - 1, self.n_fft, window, self.hop_length, phase).to(ceps.device)
        y = cep_filter(pulses, AudioTensor(ceps, self.hop_length)).as_tensor()
        if log_mag is None:
            return AudioTensor(y)
        if noise is None:
            noise = torch.randn_like(pulses.as_tensor())
        elif isinstance(noise, AudioTensor):
            assert noise.hop_length == 1, f"the noise must be at hop 1 (got {noise.hop_length})"
            noise = noise.as_tensor()
        v = LTVZeroPhaseFIRFilter(window)(AudioTensor(noise), AudioTensor(log_mag, self.hop_length)).as_tensor()
        n = min(y.shape[1], v.shape[1])
        return AudioTensor(y[:, :n] + v[:, :n])
