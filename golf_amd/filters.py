"""Drop-in LPC synthesis filters (reference models/filters.py:52-195), MI355X-native.

Same class names, constructor arguments, ``forward`` / ``reverse`` signatures and ``.ctrl`` protocol
as the reference, so ``class_path: golf_amd.filters.LTVMinimumPhaseFilterPrecise`` replaces
``models.filters.LTVMinimumPhaseFilterPrecise`` in a GOLF YAML config.  The filters own no parameters
or persistent buffers (state_dict compatible with reference checkpoints).
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import functional as GF
from .audiotensor import AudioTensor
from .ctrl import Controllable, wrap_ctrl_fn
from .utils import biquads2lpc, get_logits2biquads, get_radiation_time_filter, get_window_fn, lsp2lpc, rc2lpc

__all__ = ["LTVCepFilter", "LTVMLSAFilter2", "DiffWorldSPFilter", "melscale_fbanks", "FilterInterface", "LTVFilterInterface", "LTVMinimumPhaseFilterPrecise", "LTVMinimumPhaseFilter",
           "LTVZeroPhaseFIRFilter", "LTVZeroPhaseFIRFilterPrecise", "LTVAPZeroPhaseFIRFilter", "LTIAcousticFilter",
           "LTVMinimumPhaseFIRFilterPrecise", "LTVMinimumPhaseFIRFilter", "LTIRadiationFilter",
           "SampleBasedLTVMinimumPhaseFilter", "convert2samplewise"]


class FilterInterface(Controllable):
    def forward(self, ex: Tensor, *args, **kwargs) -> Tensor:
        raise NotImplementedError


class LTVFilterInterface(FilterInterface):
    def forward(self, ex: AudioTensor, *args, **kwargs) -> AudioTensor:
        raise NotImplementedError

    def reverse(self, ex: AudioTensor, *args, **kwargs) -> AudioTensor:
        raise NotImplementedError


def _check_filter_inputs(ex: AudioTensor, gain: AudioTensor, a: AudioTensor) -> int:
    assert ex.ndim == 2, ex.shape
    assert gain.ndim == 2, gain.shape
    assert a.ndim == 3, a.shape
    assert a.shape[1] == gain.shape[1], (a.shape, gain.shape)
    assert ex.hop_length == 1, f"excitation must be at hop 1 (got {ex.hop_length})"
    assert gain.hop_length == a.hop_length, (gain.hop_length, a.hop_length)
    return int(gain.hop_length)


class LTVMinimumPhaseFilterPrecise(LTVFilterInterface):
    """GOLF-ss end filter: sample-wise time-varying all-pole filter with frame-rate controls
    (reference models/filters.py:64-113).  ``forward`` runs golf_ltv_allpole_{fwd,bwd}_f32; float64 AudioTensors run the
    float64 recursion (golf_ltv_allpole_{fwd,bwd}_f64) and come back as float64."""

    # "fp64", set per instance (``model.decoder.end_filter.precision = "fp64"``): fp32 tensors through the float64 recursion
    # (functional.ltv_allpole_ss(mode="fp64")) -- for the utterances at the edge of stability, a parity check, a render
    # that has to be right; one serial recursion per utterance instead of the time-chunked scan.  Any other value raises.
    precision = "fp32"

    def __init__(self, lpc_order: int = None, lpc_parameterisation: str = "rc2lpc", max_abs_value: float = 1.0):
        super().__init__()
        if lpc_parameterisation in ("coef", "conj", "real"):
            to_biquads = get_logits2biquads(lpc_parameterisation, max_abs_value)

            def logits2lpc(logits: Tensor) -> Tensor:
                if logits.is_cuda and logits.shape[-1] <= 64 and logits.shape[-1] % 2 == 0:   # one fused kernel
                    return GF.biquad_logits2lpc(logits, lpc_parameterisation, max_abs_value)
                return biquads2lpc(to_biquads(logits.view(logits.shape[0], logits.shape[1], -1, 2)))

            num_logits = lpc_order
        elif lpc_parameterisation == "rc2lpc":
            def logits2lpc(logits: Tensor) -> Tensor:
                if logits.is_cuda and logits.shape[-1] <= 64:   # one fused kernel instead of ~100 tiny ones
                    return GF.rc2lpc_logits(logits, max_abs_value)
                return rc2lpc(torch.tanh(logits) * max_abs_value)   # host-side protocol logic (CPU tensors)

            num_logits = lpc_order
        elif lpc_parameterisation == "lsp2lpc":
            # softmax -> cumulative sum: M+1 increasing values ending at 1; rolled so that the 1 (-> pi) sits in the gain
            # slot and the other M are interlaced line spectral frequencies on (0, pi) (models/filters.py:82-86)
            def logits2lpc(logits: Tensor) -> Tensor:
                return lsp2lpc(logits.softmax(-1).cumsum(-1).roll(1, -1) * torch.pi)[..., 1:]

            num_logits = lpc_order + 1
        else:
            raise ValueError(f"Unknown lpc_parameterisation: {lpc_parameterisation}")
        self.logits2lpc = logits2lpc
        if lpc_order is not None:
            self.ctrl = wrap_ctrl_fn(
                split_size=(1, num_logits),
                trsfm_fn=lambda log_gain, lpc_logits: (
                    torch.exp(log_gain),
                    lpc_logits.new_tensor(logits2lpc(lpc_logits.as_tensor())),
                ),
            )

    def prefetch(self, gain: AudioTensor, a: AudioTensor, n_samples: int = None, overlap: bool = True) -> None:
        """Optional hook (not in the reference): start the excitation-independent phase of the filter — the
        per-chunk transition matrices — as soon as the coefficients are known, optionally on a second HIP stream.
        ``SourceFilterSynth(overlap_prefetch=True)`` calls it; ``forward`` picks the result up if shapes match."""
        hop = int(a.hop_length)
        F = a.shape[1]
        T = (F - 1) * hop + 1 if n_samples is None else min(int(n_samples), (F - 1) * hop + 1)
        # the fp32 matrices of the inference path serve training too (ABI 3: the backward runs its own refinement sweep);
        # with grad mode on the handle also keeps what the backward reads -- whichever decoder input ends up requiring a
        # gradient (a frozen filter under a trainable source included: ADVICE r2), the forward can pick it up
        if self.precision != "fp32" or a.as_tensor().dtype == torch.float64:
            return   # the float64 recursion has no excitation-independent phase
        self._prepared = GF.ltv_allpole_prepare(a.as_tensor(), hop, T, overlap=overlap, fast=True,
                                                training=torch.is_grad_enabled())

    # Health monitor (not in the reference).  The filter reports, per forward, how many utterances needed their
    # chunk maps recomputed, whether a non-finite sample left it and whether a bounded device-side wait ran out
    # (include/golf_amd.h golf_ltv_allpole_status_u32).  With ``health_check = True`` every eager forward queues those four
    # words for an asynchronous copy to pinned host memory and the NEXT forward (or ``health()``) looks at the ones that have
    # arrived: no synchronisation, one tiny kernel + 16 bytes per call.  Off while a hipGraph is being captured.
    health_check = False

    def health(self, wait: bool = False) -> dict:
        """Status words of the most recent monitored forward that has reached the host (``wait=True``: synchronise on all that
        are queued).  Every monitored forward is looked at exactly once -- the pending copies wait in a queue (a GPU-bound loop
        runs ahead of the device, so a single slot overwritten per call dropped every status but the last: ADVICE r4) -- and
        this is the one place that warns about a fix-up timeout, a scan mismatch or non-finite output."""
        import warnings

        q = self.__dict__.setdefault("_health_queue", [])
        while q:
            host, ev = q[0]
            if wait:
                ev.synchronize()
            if not ev.query():
                break
            q.pop(0)
            self._health_last = w = GF.ss_status(host, warn=False)
            bad = [k for k in ("fixup_timeout", "scan_mismatch", "nonfinite") if w[k]]
            if bad:
                warnings.warn(f"golf_amd: sample-wise LPC filter reported {', '.join(bad)} (status {w})", RuntimeWarning)
        return getattr(self, "_health_last", None)

    def forward(self, ex: AudioTensor, gain: AudioTensor, a: AudioTensor, zi: Tensor = None, return_zf: bool = False):
        """``zi``: optional initial state, a plain (B, M) tensor with y[b, -1-j] = zi[b, j]; ``return_zf=True`` returns
        ``(AudioTensor, zf)`` with zf (B, M) the final state -- the ``zi`` of the segment that follows, differentiable
        (not in the reference module; torchlpc.sample_wise_lpc's ``zi``).  Without them: the reference's call."""
        hop = _check_filter_inputs(ex, gain, a)
        if self.precision not in ("fp32", "fp64"):
            raise ValueError(f"{type(self).__name__}.precision must be 'fp32' or 'fp64' (got {self.precision!r})")
        prepared, self._prepared = getattr(self, "_prepared", None), None
        x = ex.as_tensor()
        mode = "fp64" if self.precision == "fp64" else None
        f64 = mode is not None or x.dtype == torch.float64   # the float64 recursion: no status words to monitor
        st = None
        if self.health_check and not f64 and x.is_cuda and not torch.cuda.is_current_stream_capturing():
            self.health()
            st = torch.zeros(4, dtype=torch.int32, device=x.device)
        if zi is None and not return_zf:
            y = GF.ltv_allpole_ss(x, gain.as_tensor(), a.as_tensor(), hop, prepared, mode=mode, status=st)
        else:
            y, zf = GF.ltv_allpole_ss(x, gain.as_tensor(), a.as_tensor(), hop, prepared, mode=mode, status=st, zi=zi,
                                      return_zf=True)
        if st is not None:
            host = torch.empty(4, dtype=torch.int32, pin_memory=True)
            host.copy_(st, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(x.device))
            q = self.__dict__.setdefault("_health_queue", [])
            q.append((host, ev))
            if len(q) > 64:      # (a caller that never comes back to look: keep the newest)
                del q[0]
        if return_zf:
            return AudioTensor(y), zf
        return AudioTensor(y)

    def reverse(self, ex: AudioTensor, y: AudioTensor, gain: AudioTensor, a: AudioTensor
                ) -> Tuple[AudioTensor, AudioTensor]:
        """Inverse filtering of a target (reference models/filters.py:186-195): returns
        (ex*gain, e) with e[t] = y[t] + sum_i up(a)[t,i] y[t-1-i]."""
        hop = int(a.hop_length)
        e = GF.ltv_inverse(y.as_tensor(), a.as_tensor(), hop)
        return ex * gain, AudioTensor(e)


class LTVMinimumPhaseFilter(LTVMinimumPhaseFilterPrecise):
    """GOLF-ff end filter: per-frame LTI all-pole + windowed overlap-add
    (reference models/filters.py:116-184); custom backward w.r.t. ex, gain and a
    (golf_lti_frames_ola_{fwd,bwd}_f32).  Runs and trains at any ``lpc_order`` up to 64, any hop and any even
    ``window_length >= 2*hop``: the recipe shapes (order <= 38, hop >= the ring width above the order, window a multiple of
    it) on the ring kernels, every other shape on the wave-per-frame kernels (``functional.ff_on_ring_grid``).  The
    streaming form (``stream.py``) keeps order <= 38."""

    def prefetch(self, *args, **kwargs) -> None:  # the frame-wise filter has no excitation-independent phase
        return None

    def __init__(self, window: str, window_length: int, centred: bool = True, **kwargs):
        super().__init__(**kwargs)
        # the reference keeps diag(window) as a non-persistent (W,1,W) conv kernel `_kernel`;
        # only its diagonal is ever used, so that is all that is stored here (also non-persistent).
        self.register_buffer("_window", get_window_fn(window)(window_length).float(), persistent=False)
        self.centred = centred

    def forward(self, ex: AudioTensor, gain: AudioTensor, a: AudioTensor) -> AudioTensor:
        hop = _check_filter_inputs(ex, gain, a)
        W = self._window.shape[0]
        assert W >= hop * 2, f"{W} < {hop * 2}"
        x = ex.as_tensor()
        if not self.centred:
            x = x[..., hop // 2:]
        y = GF.lti_frames_ola(x, gain.as_tensor(), a.as_tensor(), self._window, hop)
        if not self.centred:
            y = torch.nn.functional.pad(y, (hop // 2, 0), "reflect")
        return AudioTensor(y)


class _LTVFIRFilter(LTVFilterInterface):
    """What the LTV FIR modules designed from log magnitudes share: the window vectors, the ``n_mag`` control split, the
    input checks and the un-windowed kernels.  Every public class with a computation of its own defines its own
    ``forward``, never a shared one that dispatches: the streams recognise the filter they can run block by block by the
    identity of that function (``stream._branch_kind``)."""

    def __init__(self, window: str, n_mag: int = None):
        super().__init__()
        self.window_fn = get_window_fn(window)
        self._windows = {}
        if n_mag is not None:
            self.ctrl = wrap_ctrl_fn(split_size=(n_mag,), trsfm_fn=lambda x: (x,))

    def _make_window(self, n: int, device) -> Tensor:
        return self.window_fn(n).to(device=device, dtype=torch.float32).contiguous()

    def _window(self, n: int, device) -> Tensor:
        key = (n, str(device))
        w = self._windows.get(key)
        if w is None:
            w = self._windows[key] = self._make_window(n, device)
        return w

    def windowing(self, kernel: Tensor) -> Tensor:
        return kernel * self._window(kernel.shape[-1], kernel.device)

    @staticmethod
    def _get_fir(design, log_mag: Tensor) -> Tensor:
        """(…,F,n_mag) -> (…,F,N) impulse responses of ``design``, *not* windowed."""
        lm = log_mag.reshape(-1, log_mag.shape[-2], log_mag.shape[-1]) if log_mag.dim() != 3 else log_mag
        n = 2 * (lm.shape[-1] - 1)
        k = GF._fir_kernels(design, lm, torch.ones(n, device=lm.device))
        return k.reshape(*log_mag.shape[:-1], n)

    def _inputs(self, ex: AudioTensor, log_mag: AudioTensor):
        assert ex.ndim == 2, ex.shape
        assert log_mag.ndim == 3, log_mag.shape
        assert ex.hop_length == 1, f"excitation must be at hop 1 (got {ex.hop_length})"
        x = ex.as_tensor()
        return x, log_mag.as_tensor(), self._window(2 * (log_mag.shape[-1] - 1), x.device), int(log_mag.hop_length)


class LTVZeroPhaseFIRFilter(_LTVFIRFilter):
    """Noise filter of every GOLF decoder: per-frame zero-phase FIR designed from log magnitudes
    (reference models/filters.py:286-306,340-384).  ``forward`` runs golf_zero_phase_fir_kernels_f32 (cosine
    transform on the matrix cores) + golf_ltv_fir_frames_{fwd,bwd}_f32; differentiable w.r.t. ``ex`` and ``log_mag``.

    ``conv_method`` ("direct" | "fft") only selected between two numerically equivalent convolution routines in the
    reference; it is accepted and validated for config compatibility, there is one kernel here."""

    def __init__(self, window: str, conv_method: str = "direct", n_mag: int = None):
        super().__init__(window=window, n_mag=n_mag)
        if conv_method not in ("direct", "fft"):
            raise ValueError(f"Unknown conv_method: {conv_method}")

    def get_zero_phase_fir(self, log_mag: Tensor) -> Tensor:
        """(…,F,n_mag) -> (…,F,N) zero-phase impulse responses, *not* windowed (filters.py:294-300)."""
        return self._get_fir(GF.ZERO_PHASE_FIR, log_mag)

    def forward(self, ex: AudioTensor, log_mag: AudioTensor) -> AudioTensor:
        return AudioTensor(GF.zero_phase_fir_filter(*self._inputs(ex, log_mag)))


class LTVZeroPhaseFIRFilterPrecise(LTVZeroPhaseFIRFilter):
    """Sample-wise variant (reference models/filters.py:286-337; what ``convert2samplewise`` swaps in): the windowed
    kernels are linearly interpolated to sample rate before the convolution.  Same kernels underneath
    (golf_ltv_fir_frames_* twice, rows f and f+1, blended per sample)."""

    def __init__(self, window: str, n_mag: int = None):
        super().__init__(window=window, conv_method="direct", n_mag=n_mag)

    def forward(self, ex: AudioTensor, log_mag: AudioTensor) -> AudioTensor:
        return AudioTensor(GF.zero_phase_fir_filter_precise(*self._inputs(ex, log_mag)))


class LTVAPZeroPhaseFIRFilter(LTVZeroPhaseFIRFilter):
    """Reference models/filters.py:387-397: same filter, sigmoid-bounded magnitudes."""

    def __init__(self, window: str, conv_method: str = "direct", n_mag: int = None):
        super().__init__(window, conv_method, n_mag)
        n_fft = 2 * (n_mag - 1)
        if n_mag is not None:
            self.ctrl = wrap_ctrl_fn(split_size=(n_mag,),
                                     trsfm_fn=lambda x: (torch.log(torch.sigmoid(x) * n_fft ** 0.5),))


class LTIAcousticFilter(FilterInterface):
    """Room filter of the GOLF decoders (reference models/filters.py:426-456): y = ex + causal FIR tail with a
    learnable ``kernel`` of ``length - 1`` taps (zeros at init => identity); same parameter name/shape as the
    reference so checkpoints load.  Runs golf_lti_fir_f32 (+ its adjoint / taps gradient)."""

    def __init__(self, length: int, conv_method: str = "direct"):
        super().__init__()
        if conv_method not in ("direct", "fft"):
            raise ValueError(f"Unknown conv_method: {conv_method}")
        self.kernel = torch.nn.Parameter(torch.zeros(length - 1))
        self._padding = length - 1
        # the constant end of the tap vector (the direct path's 1 + zeros up to a multiple of 4 taps): a buffer, so that
        # building the taps is one concatenation instead of two fills and a concatenation per call
        self.register_buffer("_tail", torch.cat([torch.ones(1), torch.zeros((-length) % 4)]), persistent=False)

    def forward(self, ex: AudioTensor) -> AudioTensor:
        K = self._padding
        taps = torch.cat([self.kernel, self._tail.to(self.kernel.dtype)])
        return AudioTensor(GF.lti_fir(ex.as_tensor(), taps, K), hop_length=ex.hop_length)

    @property
    def impulse_response(self) -> Tensor:
        return torch.cat([self.kernel, torch.ones(1, device=self.kernel.device)]).flip(0)


class LTVMinimumPhaseFIRFilterPrecise(_LTVFIRFilter):
    """Sample-wise minimum-phase FIR filter (reference models/filters.py:198-241): per-frame minimum-phase impulse
    responses designed from log magnitudes (same magnitude response as the zero-phase filter, response from tap 0, no
    lookahead), linearly interpolated to sample rate, y[t] = sum_j h_t[j] ex[t-j].  ``forward`` runs
    golf_min_phase_fir_kernels_f32 (two contractions on the matrix cores) + golf_ltv_fir_frames_causal_* twice (rows f and
    f+1, blended per sample); differentiable w.r.t. ``ex`` and ``log_mag``.

    ``n_mag`` (not in the reference's signature; the zero-phase twin has it too) installs the ``.ctrl`` split that lets
    the class sit in a decoder."""

    def _make_window(self, n: int, device) -> Tensor:
        return GF.min_phase_window(self.window_fn, n, device)

    @staticmethod
    def get_minimum_phase_fir(log_mag: Tensor) -> Tensor:
        """(…,F,n_mag) -> (…,F,N) minimum-phase impulse responses, *not* windowed (filters.py:203-214)."""
        return _LTVFIRFilter._get_fir(GF.MIN_PHASE_FIR, log_mag)

    def forward(self, ex: AudioTensor, log_mag: AudioTensor) -> AudioTensor:
        return AudioTensor(GF.min_phase_fir_filter_precise(*self._inputs(ex, log_mag)))


class LTVMinimumPhaseFIRFilter(LTVMinimumPhaseFIRFilterPrecise):
    """Frame-wise minimum-phase FIR filter (reference models/filters.py:244-283): frame f's kernel filters its hop
    samples, y[f*hop+n] = sum_j h_f[j] ex[f*hop+n-j], T // hop frames (more than there are kernels is an error, as in the
    reference).  golf_min_phase_fir_kernels_f32 + golf_ltv_fir_frames_causal_{fwd,bwd}_f32.

    ``conv_method`` ("direct" | "fft") is accepted and validated for config compatibility, as in the zero-phase twin."""

    def __init__(self, window: str, conv_method: str = "direct", n_mag: int = None):
        super().__init__(window=window, n_mag=n_mag)
        if conv_method not in ("direct", "fft"):
            raise ValueError(f"Unknown conv_method: {conv_method}")

    def forward(self, ex: AudioTensor, log_mag: AudioTensor) -> AudioTensor:
        return AudioTensor(GF.min_phase_fir_filter(*self._inputs(ex, log_mag)))


class LTIRadiationFilter(FilterInterface):
    """Lip-radiation filter (reference models/filters.py:400-423): a fixed FIR of 2*num_zeros + 1 taps, same-length
    output, y[t] = sum_i r[i] ex[t + num_zeros - i] with r = get_radiation_time_filter(num_zeros, window).  ``_kernel``
    is the reference's non-persistent (1, 1, 2*num_zeros+1) buffer (r flipped: a correlation kernel).  Runs
    golf_lti_fir_f32; the gradient goes to ``ex`` only."""

    def __init__(self, num_zeros: int, window: str = "hanning"):
        super().__init__()
        k = get_radiation_time_filter(num_zeros, get_window_fn(window)).flip(0).float()
        self.register_buffer("_kernel", k.unsqueeze(0).unsqueeze(0), persistent=False)
        self._padding = k.shape[0] // 2
        # the kernel of golf_lti_fir_f32 holds a multiple of 4 taps: zeros behind the last one
        self.register_buffer("_taps", torch.cat([k, torch.zeros((-k.shape[0]) % 4)]), persistent=False)

    def forward(self, ex: Tensor) -> Tensor:
        assert ex.ndim == 2
        if isinstance(ex, AudioTensor):
            return AudioTensor(GF.lti_fir(ex.as_tensor(), self._taps, self._padding), hop_length=ex.hop_length)
        return GF.lti_fir(ex, self._taps, self._padding)


class SampleBasedLTVMinimumPhaseFilter(LTVMinimumPhaseFilter):
    """Deprecated alias of the sample-wise all-pole filter (reference models/filters.py:763-790): the reference upsamples
    the coefficients and calls sample_wise_lpc, which is what ``LTVMinimumPhaseFilterPrecise.forward`` runs on the
    frame-rate tracks."""

    def __init__(self, lpc_order: int = None, lpc_parameterisation: str = "rc2lpc", max_abs_value: float = 1, **kwargs):
        import warnings

        warnings.warn("SampleBasedLTVMinimumPhaseFilter is deprecated. Use LTVMinimumPhaseFilterPrecise instead.")
        super().__init__("hanning", 1, lpc_order=lpc_order, lpc_parameterisation=lpc_parameterisation,
                         max_abs_value=max_abs_value)

    prefetch = LTVMinimumPhaseFilterPrecise.prefetch
    forward = LTVMinimumPhaseFilterPrecise.forward


def _on_hip_frames(module, x: Tensor, ctrl: Tensor) -> bool:
    """Whether an STFT-domain filter module runs ``GF.stft_filter_frames`` on these inputs: not switched off
    (``hip_frames``), ROCm device tensors in fp32 (or fp16 / bf16 under autocast), and a geometry the kernel takes -- centred,
    n_fft a power of two in [64, 2048], n_fft >= 2*hop, more than n_fft/2 samples, at least two frames.  Everything else
    (CPU tensors, float64, center=False, n_fft = 1000 ...) runs torch.stft / torch.istft."""
    if not (module.hip_frames and x.is_cuda and ctrl.is_cuda and getattr(module, "center", True)):
        return False
    dtypes = (torch.float32, torch.float16, torch.bfloat16) if torch.is_autocast_enabled() else (torch.float32,)
    if x.dtype not in dtypes or ctrl.dtype not in dtypes:
        return False
    n, hop = int(module.n_fft), int(module.hop_length)
    frames = min(1 + x.shape[-1] // hop, ctrl.shape[1])
    return n & (n - 1) == 0 and 64 <= n <= 2048 and n >= 2 * hop and x.shape[-1] > n // 2 and frames >= 2


def _hip_frames(module, x: Tensor, ctrl: Tensor) -> AudioTensor:
    """The module's response rows on bins 0 .. n_fft/2 (torch, fp32, differentiable) through ``GF.stft_filter_frames``."""
    with torch.autocast("cuda", enabled=False):
        H = module.response_rows(ctrl.float())
        return AudioTensor(GF.stft_filter_frames(x.float(), H, module._window, module.hop_length))


class LTVCepFilter(LTVFilterInterface):
    """Cepstral harmonic filter of the NHV baseline (reference models/filters.py:559-623; cfg/ae/decoder/nhv.yaml):
    ``filter_order + 1`` cepstral coefficients per frame -> log-magnitude response (even extension + FFT) -> zero- or
    minimum-phase frequency response (the minimum phase is minus the Hilbert transform of the log magnitude) -> applied
    in the STFT domain (two-sided STFT with ``window``, multiply, inverse STFT).

    On a ROCm device the STFT-domain part runs and trains on the frame-filter kernel (``GF.stft_filter_frames``: the
    arithmetic of the streamed decoder, custom backward) for fp32 inputs -- fp16 / bf16 under autocast -- when n_fft is a
    power of two in [64, 2048], n_fft >= 2*hop, the input is longer than n_fft/2 and there are at least two frames; the
    response rows (cepstra -> bins 0 .. n_fft/2, complex for "min", real for "zero") stay torch autograd.  CPU tensors,
    float64 and every other geometry run stock PyTorch on rocFFT, as does an instance with ``hip_frames = False``; both paths
    return hop*(frames-1) samples.  The reference takes the transforms from torchaudio (third party); the stock path makes
    the same torch.stft / torch.istft calls directly.  No fused design kernel (cepstrum -> response) exists.

    ``envelope.SpectralEnvelopeAnalysis(sample_rate, hop_length, n_fft, filter_order)`` measures ``ceps`` on a recording with
    a known f0 track, in this filter's convention (log|H|[k] = c_0 + 2 sum_{m>=1} c_m cos(2 pi k m / n_fft)), and its
    ``synthesise`` runs the copy-synthesis through this module."""

    hip_frames = True   # False: torch.stft / torch.istft on the device too

    def __init__(self, filter_order: int, n_fft: int, window: str, hop_length: int, phase: str = "zero", **kwargs):
        super().__init__()
        if n_fft % 2 or phase not in ("zero", "min"):
            raise ValueError("LTVCepFilter: n_fft must be even and phase 'zero' or 'min'")
        # saved configs spell out the transform defaults (ckpts/interspeech24/nhv/config.yaml); anything else is refused
        defaults = {"win_length": None, "pad": 0, "normalized": False, "wkwargs": None, "pad_mode": "reflect"}
        odd = {k: v for k, v in kwargs.items() if k not in defaults or (v != defaults[k] and not (k == "win_length" and v == n_fft))}
        if odd:
            raise NotImplementedError(f"LTVCepFilter: unsupported transform arguments {odd}")
        self.n_fft, self.filter_order, self.hop_length, self.phase = n_fft, filter_order, hop_length, phase
        self.register_buffer("_window", get_window_fn(window)(n_fft).float(), persistent=False)
        self.ctrl = wrap_ctrl_fn(split_size=(filter_order + 1,), trsfm_fn=lambda x: (x,))

    def frequency_response(self, ceps: Tensor) -> Tensor:
        """(B, F, order + 1) cepstra -> (B, n_fft, F) complex (or real, phase 'zero') two-sided response."""
        n = self.n_fft
        half = torch.nn.functional.pad(ceps, (0, n // 2 - self.filter_order))          # c_0 .. c_{n/2}
        sym = torch.cat([half, half[..., 1:-1].flip(-1)], dim=-1)                       # even extension, length n
        log_mag = torch.fft.fft(sym, dim=-1).real
        if self.phase == "zero":
            return torch.exp(log_mag).transpose(-1, -2)
        # analytic signal of the log magnitude along frequency: its imaginary part is the Hilbert transform
        weights = log_mag.new_zeros(n)
        weights[0] = weights[n // 2] = 1
        weights[1: n // 2] = 2
        analytic = torch.fft.ifft(torch.fft.fft(log_mag, dim=-1) * weights, dim=-1)
        return torch.exp(torch.complex(log_mag, -analytic.imag)).transpose(-1, -2)

    def response_rows(self, ceps: Tensor) -> Tensor:
        """(B, F, order + 1) cepstra -> (B, F, n_fft/2 + 1) response rows on bins 0 .. n_fft/2, as the stream forms them."""
        return self.frequency_response(ceps)[:, : self.n_fft // 2 + 1].transpose(1, 2).contiguous()

    def forward(self, ex: AudioTensor, ceps: AudioTensor, **kwargs) -> AudioTensor:
        assert ceps.hop_length == self.hop_length
        x = ex.as_tensor()
        if _on_hip_frames(self, x, ceps.as_tensor()):
            return _hip_frames(self, x, ceps.as_tensor())
        H = self.frequency_response(ceps.as_tensor())
        X = torch.stft(x, self.n_fft, self.hop_length, self.n_fft, self._window, center=True, pad_mode="reflect",
                       normalized=False, onesided=False, return_complex=True)
        frames = min(X.shape[-1], H.shape[-1])
        Y = X[..., :frames] * H[..., :frames]
        y = torch.istft(Y, self.n_fft, self.hop_length, self.n_fft, self._window, center=True, normalized=False,
                        onesided=False, return_complex=False)
        return AudioTensor(y)


class LTVMLSAFilter2(LTVFilterInterface):
    """Mel-cepstral filter of the MLSA baseline in its STFT-domain form (reference models/filters.py:626-684): ``filter_order
    + 1`` mel cepstral coefficients per frame -> complex minimum-phase response on the frequencies warped by ``alpha`` ->
    applied in the STFT domain, with the framing of ``LTVCepFilter`` (two-sided STFT with ``window``, multiply, inverse STFT,
    hop*(frames-1) samples).  The response is the package's definition (include/golf_amd.h): H_k = exp(sum_m mc[m]
    e^{-j m theta_k}), whose imaginary exponent is the minimum phase because the warped cepstrum is causal.  The reference
    truncates the warped cepstrum at order n_fft/2 and takes the phase from a discrete Hilbert transform; the two agree to
    5e-15 in log H for n_fft >= 256, and below that this definition is the specification.  Only ``gamma = 0``.

    On a ROCm device the response rows come from the design kernel (``GF.mel_cepstrum_response``:
    golf_mlsa_response_rows_{,bwd_}f32, differentiable) and the STFT-domain part runs on the frame-filter kernel, under the
    conditions given for ``LTVCepFilter`` plus ``filter_order <= 64``.  CPU tensors, float64 and every other geometry run the
    same definition in plain torch and torch.stft / torch.istft, as does an instance with ``hip_frames = False``.

    A standalone class: the reference derives it from ``LTVMLSAFilter``, whose own framing lives in diffsptk and has no
    counterpart here (``config.mlsa_to_stft_filter`` rewrites such a config to this class, as an explicit opt-in).

    ``fit`` is the analysis counterpart: with ``envelope.SpectralEnvelopeAnalysis(..., filter_order=None)``, which returns the
    log envelope, ``fit(log_env)`` gives the ``mc`` this filter takes."""

    hip_frames = True   # False: torch.stft / torch.istft on the device too

    def __init__(self, n_fft: int, frame_period: int, filter_order: int, *args, window: str = "hanning", alpha: float = 0,
                 gamma: float = 0, **kwargs):
        super().__init__()
        if args:
            raise NotImplementedError(f"LTVMLSAFilter2: unsupported positional arguments {args}")
        if gamma != 0:
            raise NotImplementedError(f"LTVMLSAFilter2: unsupported gamma={gamma} (only gamma = 0, the plain mel cepstrum)")
        # saved configs spell out the MLSA defaults (ckpts/interspeech24/mlsa/config.yaml); anything else is refused
        defaults = {"c": None, "ignore_gain": False, "phase": "minimum", "mode": "freq-domain", "frame_length": n_fft,
                    "fft_length": n_fft}
        odd = {k: v for k, v in kwargs.items() if k not in defaults or v != defaults[k]}
        if odd:
            raise NotImplementedError(f"LTVMLSAFilter2: unsupported MLSA arguments {odd}")
        if n_fft % 2 or filter_order < 0 or not -1 < alpha < 1:
            raise ValueError("LTVMLSAFilter2: n_fft must be even, filter_order >= 0 and |alpha| < 1")
        self.n_fft, self.hop_length, self.filter_order, self.alpha = n_fft, frame_period, filter_order, float(alpha)
        window_fn = get_window_fn(window)
        try:
            w64 = window_fn(n_fft, dtype=torch.float64)
        except TypeError:   # a scipy window: float64 already
            w64 = window_fn(n_fft).double()
        self.register_buffer("_window", w64.float(), persistent=False)
        # evaluated in float64 for the float64 path (``.double()`` on the module would only widen the fp32 values)
        self.register_buffer("_window64", w64, persistent=False)
        # the design kernel's basis: this module's own, built on first device use (no process-wide cache)
        self.register_buffer("_basis", None, persistent=False)
        self.ctrl = wrap_ctrl_fn(split_size=(filter_order + 1,), trsfm_fn=lambda x: (x,))

    def _response_basis(self, mc: Tensor):
        """The kernel's basis on ``mc``'s device, or None where ``GF.mel_cepstrum_response`` runs torch.  Built once per
        device and synchronously, so that a later use on any stream is ordered after the build."""
        if not (mc.is_cuda and mc.dtype in (torch.float32, torch.float16, torch.bfloat16)
                and GF.mel_cepstrum_kernel_takes(self.n_fft, self.filter_order, self.alpha)):
            return None
        b = self._basis
        if b is None or b.device != mc.device or b.dtype != torch.float32:
            b = GF.mel_cepstrum_basis(self.n_fft, self.filter_order, self.alpha, mc.device)
            torch.cuda.current_stream(mc.device).synchronize()
            self._basis = b
        return b

    def response_rows(self, mc: Tensor) -> Tensor:
        """(B, F, order + 1) mel cepstra -> (B, F, n_fft/2 + 1) complex response rows on bins 0 .. n_fft/2."""
        if mc.shape[-1] != self.filter_order + 1:
            raise ValueError(f"LTVMLSAFilter2: {mc.shape[-1]} coefficients per frame, expected {self.filter_order + 1}")
        return GF.mel_cepstrum_response(mc, self.n_fft, self.alpha, basis=self._response_basis(mc))

    def frequency_response(self, mc: Tensor) -> Tensor:
        """(B, F, order + 1) mel cepstra -> (B, n_fft, F) complex two-sided response (Hermitian extension of the rows)."""
        H = self.response_rows(mc)
        return torch.cat([H, H[..., 1:-1].flip(-1).conj()], dim=-1).transpose(-1, -2)

    def forward(self, ex: AudioTensor, mc: AudioTensor, **kwargs) -> AudioTensor:
        assert mc.hop_length == self.hop_length
        x = ex.as_tensor()
        if _on_hip_frames(self, x, mc.as_tensor()):
            return _hip_frames(self, x, mc.as_tensor())
        H = self.frequency_response(mc.as_tensor())
        window = self._window64.to(x.dtype) if x.dtype == torch.float64 else self._window.to(x.dtype)
        X = torch.stft(x, self.n_fft, self.hop_length, self.n_fft, window, center=True, pad_mode="reflect",
                       normalized=False, onesided=False, return_complex=True)
        frames = min(X.shape[-1], H.shape[-1])
        Y = X[..., :frames] * H[..., :frames]
        y = torch.istft(Y, self.n_fft, self.hop_length, self.n_fft, window, center=True, normalized=False,
                        onesided=False, return_complex=False)
        return AudioTensor(y)

    def fit(self, log_env: Tensor) -> Tensor:
        """Least-squares mel cepstrum of natural-log magnitude rows: (B, F, n_fft/2 + 1) -> (B, F, order + 1), the ``mc``
        whose log|H| = sum_m mc[m] cos(m theta_k) is closest to ``log_env`` under the Hermitian bin weights 1, 2, .., 2, 1.
        Solved in float64, returned in ``log_env``'s dtype; plain torch, differentiable.  Meant for n_fft >= 512: the warped
        cosines are well conditioned there (condition number 2.9 at n_fft 1024, order 24, alpha 0.46; 7.8 at 2048, 64, 0.77)
        and nearly dependent on a coarse grid (4.6e9 at n_fft 64, order 24, alpha 0.46)."""
        if log_env.shape[-1] != self.n_fft // 2 + 1:
            raise ValueError(f"LTVMLSAFilter2.fit: {log_env.shape[-1]} bins, expected {self.n_fft // 2 + 1}")
        c, _ = GF.mel_cepstrum_tables(self.n_fft, self.filter_order, self.alpha, torch.float64, log_env.device)
        w = torch.full((c.shape[1], 1), 2.0, dtype=torch.float64, device=log_env.device).sqrt()
        w[0] = w[-1] = 1.0
        rows = log_env.double().reshape(-1, c.shape[1]).t() * w                       # (bins, B*F)
        mc = torch.linalg.lstsq(c.t() * w, rows).solution                               # (order + 1, B*F)
        return mc.t().reshape(*log_env.shape[:-1], self.filter_order + 1).to(log_env.dtype)


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int, norm=None,
                    mel_scale: str = "htk") -> Tensor:
    """Triangular mel filterbank (n_freqs, n_mels) — the published definition torchaudio.functional.melscale_fbanks
    implements (third party, absent here): HTK mel scale m = 2595 log10(1 + f / 700), n_mels + 2 equally spaced mel
    points, triangles between neighbouring points evaluated on linspace(0, sample_rate // 2, n_freqs)."""
    if mel_scale != "htk" or norm is not None:
        raise NotImplementedError("melscale_fbanks: only mel_scale='htk', norm=None (what the shipped configs use)")
    freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    to_mel = lambda f: 2595.0 * torch.log10(1.0 + torch.as_tensor(f, dtype=torch.float64) / 700.0)
    pts = 700.0 * (10.0 ** (torch.linspace(float(to_mel(f_min)), float(to_mel(f_max)), n_mels + 2,
                                           dtype=torch.float64) / 2595.0) - 1.0)
    width = pts[1:] - pts[:-1]
    slope = pts.unsqueeze(0) - freqs.unsqueeze(1)                       # (n_freqs, n_mels + 2)
    rising, falling = -slope[:, :-2] / width[:-1], slope[:, 2:] / width[1:]
    return torch.clamp(torch.minimum(rising, falling), min=0).float()


class DiffWorldSPFilter(LTVFilterInterface):
    """Spectral-envelope filter of the WORLD baseline (reference models/filters.py:717-760; cfg/ae/decoder/world.yaml): a
    mel spectral envelope per frame -> linear magnitudes through the rectified pseudo-inverse of a mel filterbank ->
    sqrt -> applied as a zero-phase gain in the STFT domain.  On a ROCm device the STFT-domain part runs and trains on the
    frame-filter kernel (``GF.stft_filter_frames``) under the conditions given for ``LTVCepFilter`` plus ``center=True``,
    the gain rows staying torch autograd; otherwise, and with ``hip_frames = False``, stock PyTorch (rocFFT) like the
    reference."""

    hip_frames = True   # False: torch.stft / torch.istft on the device too

    def __init__(self, n_mels: int, n_fft: int, hop_length: int, f_min: float, f_max: float, center: bool = True,
                 window: str = "hanning", **kwargs):
        super().__init__()
        fb = melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, **kwargs)
        self.register_buffer("fb", torch.linalg.pinv(fb).relu(), persistent=False)      # (n_mels, n_fft // 2 + 1)
        self.register_buffer("_window", get_window_fn(window)(n_fft).float(), persistent=False)
        self.n_fft, self.hop_length, self.center = n_fft, hop_length, center
        self.ctrl = wrap_ctrl_fn(split_size=(n_mels,), trsfm_fn=lambda x: (torch.exp(x),))

    def response_rows(self, mel_sp: Tensor) -> Tensor:
        """(B, F, n_mels) mel envelope -> (B, F, n_fft/2 + 1) real gain rows, as the stream forms them."""
        return torch.sqrt(mel_sp @ self.fb)

    def forward(self, ex: AudioTensor, mel_sp: AudioTensor) -> AudioTensor:
        assert mel_sp.hop_length == self.hop_length
        if _on_hip_frames(self, ex.as_tensor(), mel_sp.as_tensor()):
            return _hip_frames(self, ex.as_tensor(), mel_sp.as_tensor())
        gain = torch.sqrt(mel_sp.as_tensor() @ self.fb).transpose(1, 2)                  # (B, bins, F)
        X = torch.stft(ex.as_tensor(), self.n_fft, self.hop_length, self.n_fft, self._window, center=self.center,
                       pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        frames = min(X.shape[-1], gain.shape[-1])
        y = torch.istft(X[..., :frames] * gain[..., :frames], self.n_fft, self.hop_length, self.n_fft, self._window,
                        center=self.center, normalized=False, onesided=True, return_complex=False)
        return AudioTensor(y)


def convert2samplewise(config: dict) -> dict:
    """Rewrite a decoder config so frame-wise filters become their sample-wise counterparts
    (reference models/filters.py:793-809; README.md:92-94)."""
    for key, value in config.items():
        if key == "class_path":
            if ".LTVMinimumPhaseFilter" in value and not value.endswith("Precise"):
                config["class_path"] = value.rsplit(".", 1)[0] + ".LTVMinimumPhaseFilterPrecise"
                for k in ("window", "window_length", "centred"):
                    config.get("init_args", {}).pop(k, None)
                return config
            if ".LTVMinimumPhaseFIRFilter" in value and not value.endswith("Precise"):
                config["class_path"] = value.rsplit(".", 1)[0] + ".LTVMinimumPhaseFIRFilterPrecise"
                config.get("init_args", {}).pop("conv_method", None)
                return config
            if ".LTVZeroPhaseFIRFilter" in value and not value.endswith("Precise"):
                config["class_path"] = value.rsplit(".", 1)[0] + ".LTVZeroPhaseFIRFilterPrecise"
                config.get("init_args", {}).pop("conv_method", None)
                return config
        elif isinstance(value, dict):
            config[key] = convert2samplewise(value)
    return config
