"""Harmonic-plus-noise analysis: the counterpart of the harmonic-plus-noise decoders' controls, as ``lpc.LPCAnalysis`` is of
the end filter's and ``f0.F0Analysis`` of the f0.

The harmonic oscillator bank (``synth.HarmonicOscillator`` and its subclasses, the source of the DDSP, NHV, WORLD, SawSing
and PULF decoders) takes an ``amplitudes`` track (B, F, K) and the noise filter beside it (``filters.LTVZeroPhaseFIRFilter``)
takes ``log_mag`` rows (B, F, n_mag); the reference has only trained encoders to produce them.  ``HarmonicNoiseAnalysis``
measures both on a recording with a known f0 track: the classical sinusoidal / harmonic-plus-noise analysis with a
pitch-adaptive window and a per-frame chirp, one HIP kernel (golf_harmonic_analysis_f32, csrc/harm_analysis.hip; the
definition is in include/golf_amd.h).
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["HarmonicNoiseAnalysis"]


class HarmonicNoiseAnalysis(nn.Module):
    """(waveform, f0) -> ``(amplitudes, log_mag)`` at hop ``hop_length``, or ``amplitudes`` alone when ``n_mag`` is None, on
    the device (no parameters, no buffers, no gradient).  Frame f is centred on sample ``f * hop_length``, the decoders'
    frame grid; ``f0`` is in Hz with 0 for unvoiced frames, as ``F0Analysis`` gives it.  The remaining arguments are those of
    ``functional.harmonic_analysis``.  ``analysis_stream.HarmonicNoiseStream`` is the block-by-block form."""

    def __init__(self, sample_rate: float, hop_length: int, num_harmonics: int, n_mag: int = None, periods: int = 4,
                 min_window: int = None, max_window: int = 2048, unvoiced_window: int = None, smooth: int = 0,
                 eps: float = 1e-12):
        super().__init__()
        self.sample_rate, self.hop_length, self.num_harmonics, self.n_mag = sample_rate, hop_length, num_harmonics, n_mag
        self.periods, self.max_window, self.smooth, self.eps = periods, max_window, smooth, eps
        self.min_window = 2 * hop_length if min_window is None else min_window
        self.unvoiced_window = 4 * hop_length if unvoiced_window is None else unvoiced_window

    def _run(self, x, f0, return_phases: bool):
        if isinstance(x, AudioTensor):
            assert x.hop_length == 1, f"the waveform must be at hop 1 (got {x.hop_length})"
            x = x.as_tensor()
        if isinstance(f0, AudioTensor):
            assert f0.hop_length == self.hop_length, f"f0 must be at hop {self.hop_length} (got {f0.hop_length})"
            f0 = f0.as_tensor()
        assert x.ndim == 2, x.shape
        assert f0.ndim == 2, f0.shape
        return GF.harmonic_analysis(x, f0, self.sample_rate, self.hop_length, self.num_harmonics, self.n_mag, self.periods,
                                    self.min_window, self.max_window, self.unvoiced_window, self.smooth, self.eps,
                                    return_phases=return_phases)

    def analyse(self, x, f0):
        """Plain tensors ``(amplitudes, phases, log_mag)`` (``(amplitudes, phases)`` when ``n_mag`` is None): amplitudes and
        sine phases in cycles at the frames' centres, each (B, F, num_harmonics), and log_mag (B, F, n_mag)."""
        return self._run(x, f0, True)

    def forward(self, x, f0):
        out = self._run(x, f0, False)
        if self.n_mag is None:
            return AudioTensor(out, self.hop_length)
        return AudioTensor(out[0], self.hop_length), AudioTensor(out[1], self.hop_length)

    def synthesise(self, f0, amplitudes, log_mag=None, noise=None, window: str = "hanning") -> AudioTensor:
        """Copy-synthesis of analysed controls on the package's own modules: ``HarmonicOscillator`` on ``f0 / sample_rate``
        and ``amplitudes``, plus, with ``log_mag``, ``LTVZeroPhaseFIRFilter(window)`` on ``noise`` (N(0, 1) drawn on the
        device when None), truncated to the shorter of the two.  The harmonics start at phase 0: the analysed phases are
        not used."""
        from .filters import LTVZeroPhaseFIRFilter
        from .synth import HarmonicOscillator

        def plain(t):
            if isinstance(t, AudioTensor):
                assert t.hop_length == self.hop_length, f"controls must be at hop {self.hop_length} (got {t.hop_length})"
                return t.as_tensor()
            return t

        f0, amplitudes, log_mag = plain(f0), plain(amplitudes), plain(log_mag)
        phase = AudioTensor(f0 / self.sample_rate, self.hop_length)
        y = HarmonicOscillator()(phase, AudioTensor(amplitudes, self.hop_length)).as_tensor()
        if log_mag is None:
            return AudioTensor(y)
        if noise is None:
            noise = torch.randn_like(y)
        elif isinstance(noise, AudioTensor):
            assert noise.hop_length == 1, f"the noise must be at hop 1 (got {noise.hop_length})"
            noise = noise.as_tensor()
        v = LTVZeroPhaseFIRFilter(window)(AudioTensor(noise), AudioTensor(log_mag, self.hop_length)).as_tensor()
        n = min(y.shape[1], v.shape[1])
        return AudioTensor(y[:, :n] + v[:, :n])
