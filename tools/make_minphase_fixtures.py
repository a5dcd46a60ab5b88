#!/usr/bin/env python
"""Generate tests/golden/g29_min_phase_fir.npz and g30_radiation_filter.npz by running the REFERENCE'S OWN code on the CPU
(test infrastructure; needs a checkout of the reference, which is imported at run time and never copied):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_minphase_fixtures.py /path/to/reference

Its third-party imports are absent, so ``sys.modules`` placeholders stand in for pyworld, torchaudio, diffsptk, torchlpc
and torch_fftconv (none of them is on the recorded path), and ``models.audiotensor.AudioTensor`` is the reference's own
``models.utils.LegacyAudioTensor`` (the submodule directory is empty).  Everything runs in float64 (the default dtype is
switched, so that the reference's own constants are float64 too); gradients are autograd's.

Recorded, per case of g29: the windowed kernels (get_minimum_phase_fir + windowing), the minimum phase of the first frame
(minus the imaginary part of hilbert() of the even extension), the frame-wise filter and the
sample-wise one (kernels upsampled by the stand-in's reduce_hop_length, then fir_filt), each with the gradients of
sum(y * gy).  ``frame_path`` / ``precise_path`` say whether the module's own forward produced y ("forward") or whether
it does not run under the stand-in and its steps were applied to plain tensors ("steps").  Every array written is an input
or an output of reference code."""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GOLF_REFERENCE", "")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
if not os.path.isdir(os.path.join(REF, "models")):
    sys.exit("usage: make_minphase_fixtures.py REFERENCE_CHECKOUT")


def _mod(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m


class _Absent(nn.Module):
    def __init__(self, *a, **k):
        super().__init__()


_none = lambda *a, **k: None
_mod("pyworld", dio=_none)
_mod("torchlpc", sample_wise_lpc=_none)
_mod("torchaudio")
_mod("torchaudio.functional", lfilter=_none, melscale_fbanks=_none)
_mod("torchaudio.transforms", Spectrogram=_Absent, InverseSpectrogram=_Absent)
_mod("torch_fftconv")
_mod("torch_fftconv.functional", fft_conv1d=torch.nn.functional.conv1d)
_mod("diffsptk", MLSA=_Absent, MelCepstralAnalysis=_Absent, MelGeneralizedCepstrumToSpectrum=_Absent, PQMF=_Absent,
     IPQMF=_Absent)
_mod("diffsptk.functional", lsp2lpc=_none)

torch.set_default_dtype(torch.float64)
sys.path.insert(0, REF)
import models.utils as ru  # noqa: E402

_mod("models.audiotensor", AudioTensor=ru.LegacyAudioTensor)
import models.filters as rf  # noqa: E402

AT = ru.LegacyAudioTensor
rng = np.random.default_rng(2929)


def save(name, **arrs):
    arrs = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrs)
    print(f"wrote {name}.npz:", {k: v.shape for k, v in arrs.items()})


def envelope(B, F, n_mag):
    """smooth spectral envelope + frame-to-frame drift, 40 dB of dynamic range (tests/test_gpu_noise_fir.py::case)"""
    base = np.cumsum(rng.normal(0, 0.25, (B, 1, n_mag)), axis=-1)
    drift = np.cumsum(rng.normal(0, 0.05, (B, F, n_mag)), axis=1)
    return (base + drift - 2.0).clip(-6, 3)


def leaf(a):
    return torch.tensor(a, dtype=torch.float64, requires_grad=True)


def grads(y, gy, *leaves):
    out = torch.autograd.grad((y * torch.as_tensor(gy)).sum(), leaves)
    return [g.detach() for g in out]


def run_frames(mod, ex, lm, hop):
    try:
        y = mod(AT(ex), AT(lm, hop_length=hop))
        return (y.as_tensor() if hasattr(y, "as_tensor") else y), "forward"
    except Exception as e:   # noqa: BLE001 -- the stand-in AudioTensor lacks what the forward calls
        print("  frame-wise forward does not run under the stand-in:", type(e).__name__, e)
    k = mod.windowing(mod.get_minimum_phase_fir(lm))
    n = k.shape[-1]
    frames = torch.nn.functional.pad(ex, (n - 1, 0)).unfold(1, n + hop - 1, hop)
    assert frames.shape[1] <= k.shape[1]
    k = k[:, : frames.shape[1]]
    y = mod.convolve_fn(frames.reshape(1, -1, frames.shape[-1]), k.reshape(-1, 1, n).flip(-1),
                        groups=k.shape[0] * k.shape[1])
    return y.view(k.shape[0], -1), "steps"


def run_precise(mod, ex, lm, hop):
    try:
        y = mod(AT(ex), AT(lm, hop_length=hop))
        return (y.as_tensor() if hasattr(y, "as_tensor") else y), "forward"
    except Exception as e:   # noqa: BLE001
        print("  sample-wise forward does not run under the stand-in:", type(e).__name__, e)
    k = mod.windowing(mod.get_minimum_phase_fir(lm))
    up = AT(k, hop_length=hop).reduce_hop_length().as_tensor()
    return ru.fir_filt(ex[:, : up.shape[1]], up[:, : ex.shape[1]]), "steps"


def g29():
    out = {}
    for tag, B, T, F, n_mag, hop, window in (("a", 2, 45, 6, 9, 8, "hanning"), ("b", 1, 60, 3, 9, 20, "hanning"),
                                             ("c", 1, 96, 4, 33, 24, "hamming")):
        ex_np, lm_np = rng.normal(0, 1, (B, T)), envelope(B, F, n_mag)
        fw = rf.LTVMinimumPhaseFIRFilter(window=window, conv_method="direct")
        pr = rf.LTVMinimumPhaseFIRFilterPrecise(window=window)
        with torch.no_grad():
            lm0 = torch.tensor(lm_np)
            kernel = fw.windowing(rf.LTVMinimumPhaseFIRFilterPrecise.get_minimum_phase_fir(lm0))
            phase = -ru.hilbert(torch.cat([lm0, lm0.flip(-1)[..., 1:-1]], dim=-1), dim=-1).imag
        ex, lm = leaf(ex_np), leaf(lm_np)
        y, path = run_frames(fw, ex, lm, hop)
        gy = rng.normal(0, 1, tuple(y.shape))
        g_ex, g_lm = grads(y, gy, ex, lm)
        ex2, lm2 = leaf(ex_np), leaf(lm_np)
        py, ppath = run_precise(pr, ex2, lm2, hop)
        pgy = rng.normal(0, 1, tuple(py.shape))
        pg_ex, pg_lm = grads(py, pgy, ex2, lm2)
        print(f"g29{tag}: frame-wise {path} {tuple(y.shape)}, sample-wise {ppath} {tuple(py.shape)}")
        out.update({f"{tag}_ex": ex_np, f"{tag}_log_mag": lm_np, f"{tag}_hop": hop, f"{tag}_window": window,
                    f"{tag}_kernel": kernel, f"{tag}_theta": phase[:, 0, :n_mag],
                    f"{tag}_y": y, f"{tag}_gy": gy, f"{tag}_g_ex": g_ex, f"{tag}_g_log_mag": g_lm,
                    f"{tag}_frame_path": path,
                    f"{tag}_p_y": py, f"{tag}_p_gy": pgy, f"{tag}_p_g_ex": pg_ex, f"{tag}_p_g_log_mag": pg_lm,
                    f"{tag}_precise_path": ppath})
    save("g29_min_phase_fir", **out)


def g30():
    out = {}
    for tag, num_zeros, window, B, T in (("a", 16, "hanning", 2, 120), ("b", 5, "hamming", 3, 47), ("c", 1, "hanning", 1, 9)):
        mod = rf.LTIRadiationFilter(num_zeros, window=window)
        taps = ru.get_radiation_time_filter(num_zeros, ru.get_window_fn(window))
        ex_np = rng.normal(0, 1, (B, T))
        ex = leaf(ex_np)
        y = mod(ex)
        gy = rng.normal(0, 1, tuple(y.shape))
        (g_ex,) = grads(y, gy, ex)
        out.update({f"{tag}_num_zeros": num_zeros, f"{tag}_window": window, f"{tag}_taps": taps,
                    f"{tag}_taps_plain": ru.get_radiation_time_filter(num_zeros), f"{tag}_module_kernel": mod._kernel,
                    f"{tag}_ex": ex_np, f"{tag}_y": y, f"{tag}_gy": gy, f"{tag}_g_ex": g_ex})
    save("g30_radiation_filter", **out)


if __name__ == "__main__":
    g29()
    g30()
