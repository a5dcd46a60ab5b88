"""f0 analysis: the counterpart of ``lpc.LPCAnalysis`` for the other input every decoder takes.

The reference reads its f0 tracks from files made with ``pyworld.dio`` (models/utils.py:596-602, scripts/wav2f0.py), a CPU
package.  ``F0Analysis`` is not that estimator: it is YIN (de Cheveigne & Kawahara, JASA 2002, steps 1-5) as one HIP kernel
(golf_f0_yin_f32, csrc/f0_yin.hip), so its tracks differ from f0 files made by the reference's scripts -- in the octave
choices of a hard frame and by the fraction of a hertz everywhere.  It keeps the reference's convention that ``f0 == 0``
marks an unvoiced frame (ltng/ae.py:98-101).
"""
from __future__ import annotations

from torch import nn

from . import functional as GF
from .audiotensor import AudioTensor

__all__ = ["F0Analysis"]


class F0Analysis(nn.Module):
    """A waveform -> its f0 track in Hz at hop ``hop_length``, 0 where unvoiced, on the device (no parameters, no buffers, no
    gradient).  ``centred=True`` puts frame f around sample ``f * hop_length`` (the decoders' frame grid,
    ``T // hop_length + 1`` frames, the grid of ``LPCAnalysis``); ``centred=False`` starts it there.  Candidates run from
    ``f0_min`` to ``f0_max``; ``window_length`` is the integration window of the difference function (default: two periods
    of ``f0_min``); a frame is voiced if its normalised difference falls below ``threshold`` and its RMS exceeds
    ``rms_floor``."""

    def __init__(self, sample_rate: float, hop_length: int, f0_min: float = 60.0, f0_max: float = 1000.0,
                 window_length: int = None, threshold: float = 0.15, rms_floor: float = 0.0, centred: bool = True):
        super().__init__()
        self.sample_rate, self.hop_length = sample_rate, hop_length
        self.f0_min, self.f0_max = f0_min, f0_max
        self.tau_min, self.tau_max, self.window_length = GF.f0_lags(sample_rate, f0_min, f0_max, window_length)
        self.threshold, self.rms_floor, self.centred = threshold, rms_floor, centred

    def _run(self, x, return_all: bool):
        if isinstance(x, AudioTensor):
            assert x.hop_length == 1, f"the waveform must be at hop 1 (got {x.hop_length})"
            x = x.as_tensor()
        assert x.ndim == 2, x.shape
        return GF.f0_yin(x, self.sample_rate, self.hop_length, self.f0_min, self.f0_max, self.window_length, self.threshold,
                         self.rms_floor, centred=self.centred, return_all=return_all)

    def analyse(self, x):
        """Plain tensors ``(f0, period, ap)``, each (B, F): Hz (0 where unvoiced), the period in samples (finite in every
        frame) and the aperiodicity, the normalised difference at that period."""
        return self._run(x, True)

    def forward(self, x) -> AudioTensor:
        return AudioTensor(self._run(x, False), self.hop_length)

    def voicing(self, x) -> AudioTensor:
        """1.0 where voiced, 0.0 elsewhere: the track ``HarmonicPlusNoiseSynth(voicing=)`` takes."""
        return AudioTensor((self._run(x, False) > 0).float(), self.hop_length)
