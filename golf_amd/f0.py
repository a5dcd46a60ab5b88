"""f0 analysis: the counterpart of ``lpc.LPCAnalysis`` for the other input every decoder takes.

The reference reads its f0 tracks from files made with ``pyworld.dio`` (models/utils.py:596-602, scripts/wav2f0.py), a CPU
package.  ``F0Analysis`` is not that estimator: it is YIN (de Cheveigne & Kawahara, JASA 2002, steps 1-5) as one HIP kernel
(golf_f0_yin_f32, csrc/f0_yin.hip), so its tracks differ from f0 files made by the reference's scripts -- in the octave
choices of a hard frame and by the fraction of a hertz everywhere.  It keeps the reference's convention that ``f0 == 0``
marks an unvoiced frame (ltng/ae.py:98-101).

``F0Tracker`` decides the utterance instead of the frame: the same difference function gives up to seven candidate periods
per frame (golf_f0_candidates_f32) and a second kernel finds the cheapest path through them and the unvoiced state
(golf_f0_viterbi_f32, csrc/f0_viterbi.hip), in the manner of Praat's path finder (Boersma 1993).
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


class F0Tracker(F0Analysis):
    """A waveform -> its f0 track by candidates and a minimum-cost path (``functional.f0_track``): the arguments of
    ``F0Analysis`` (``threshold`` is kept for the base class and plays no part in the path), ``n_candidates`` per frame
    (1..7) and the four costs of ``functional.f0_viterbi``, whose defaults are Praat's moved to the scale of d' and not tuned
    on speech.  ``forward`` and ``voicing`` are those of the base class on the tracked path."""

    def __init__(self, sample_rate: float, hop_length: int, f0_min: float = 60.0, f0_max: float = 1000.0,
                 window_length: int = None, threshold: float = 0.15, rms_floor: float = 0.0, centred: bool = True,
                 n_candidates: int = 7, unvoiced_cost: float = 0.3, lag_cost: float = 0.02, jump_cost: float = 0.35,
                 switch_cost: float = 0.14):
        super().__init__(sample_rate, hop_length, f0_min, f0_max, window_length, threshold, rms_floor, centred)
        self.n_candidates = n_candidates
        self.unvoiced_cost, self.lag_cost, self.jump_cost, self.switch_cost = unvoiced_cost, lag_cost, jump_cost, switch_cost

    def _run(self, x, return_all: bool):
        if isinstance(x, AudioTensor):
            assert x.hop_length == 1, f"the waveform must be at hop 1 (got {x.hop_length})"
            x = x.as_tensor()
        assert x.ndim == 2, x.shape
        return GF.f0_track(x, self.sample_rate, self.hop_length, self.f0_min, self.f0_max, self.window_length,
                           self.n_candidates, self.rms_floor, self.centred, None, self.unvoiced_cost, self.lag_cost,
                           self.jump_cost, self.switch_cost, return_all=return_all)

    def analyse(self, x):
        """Plain tensors ``(f0, state, cand_period, cand_ap)``: Hz (0 where the path is unvoiced) and the state (0 unvoiced,
        k + 1 for slot k), each (B, F), and the candidates (B, F, n_candidates)."""
        return self._run(x, True)
