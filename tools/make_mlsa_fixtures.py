#!/usr/bin/env python
"""Generate tests/golden/g31_mlsa_filter.npz and g31_mlsa_config.json by running the REFERENCE'S OWN
``models.filters.LTVMLSAFilter2.forward`` on the CPU in float64 (test infrastructure; needs a checkout of the reference,
which is imported at run time and never copied):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_mlsa_fixtures.py /path/to/reference

Its third-party imports are absent, so ``sys.modules`` placeholders stand in, as in tools/make_minphase_fixtures.py.  Three of
them are on the recorded path and are restated here from their published definitions:

* ``torchaudio.transforms.Spectrogram`` / ``InverseSpectrogram`` := torch.stft / torch.istft with torchaudio's documented
  arguments and defaults (as oracle/make_fixtures.py does for g21);
* ``diffsptk.MelGeneralizedCepstrumToSpectrum(..., out_format="log-magnitude")`` := the published procedure in float64:
  frequency transform of the mel cepstrum from ``alpha`` to 0 up to order fft_length/2 (Tokuda's recursion, applied to unit
  vectors so that it is one matrix), zero-padding to fft_length, rfft, real part;
* ``diffsptk.MLSA`` := an inert module that keeps ``frame_period`` (the reference's forward asserts on it, nothing else).

Everything else -- the even extension, ``hilbert()``, exp, the STFT-domain product, the inverse transform -- is the reference's
own code.  Recorded per case: ex, mc, y and autograd's gradients of sum(y * gy).  The config file is the parsed ``model:``
section of ckpts/interspeech24/mlsa/config.yaml: settings only."""
import json
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
    sys.exit("usage: make_mlsa_fixtures.py REFERENCE_CHECKOUT")


def _mod(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m


class _Absent(nn.Module):
    def __init__(self, *a, **k):
        super().__init__()


class _STFTBase(nn.Module):
    def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, power=2.0,
                 normalized=False, wkwargs=None, center=True, pad_mode="reflect", onesided=True):
        super().__init__()
        assert pad == 0 and not normalized
        self.n_fft = n_fft
        self.win_length = n_fft if win_length is None else win_length
        self.hop_length = self.win_length // 2 if hop_length is None else hop_length
        self.power, self.center, self.pad_mode, self.onesided = power, center, pad_mode, onesided
        self.register_buffer("window", window_fn(self.win_length, **(wkwargs or {})))


class Spectrogram(_STFTBase):
    def forward(self, x):
        assert self.power is None
        return torch.stft(x, self.n_fft, self.hop_length, self.win_length, self.window.to(x.dtype), center=self.center,
                          pad_mode=self.pad_mode, normalized=False, onesided=self.onesided, return_complex=True)


class InverseSpectrogram(_STFTBase):
    def forward(self, z, length=None):
        return torch.istft(z, self.n_fft, self.hop_length, self.win_length, self.window.to(z.real.dtype), center=self.center,
                           normalized=False, onesided=self.onesided, length=length, return_complex=False)


def freqt_matrix(in_order: int, out_order: int, a: float) -> np.ndarray:
    """(out_order + 1, in_order + 1) matrix of the frequency transform with all-pass constant ``a``: the published
    recursion run on every unit vector."""
    A = np.zeros((out_order + 1, in_order + 1))
    for col in range(in_order + 1):
        c1 = np.zeros(in_order + 1)
        c1[col] = 1.0
        g = np.zeros(out_order + 1)
        for i in range(in_order, -1, -1):
            d = g.copy()
            g[0] = c1[i] + a * d[0]
            if out_order >= 1:
                g[1] = (1.0 - a * a) * d[0] + a * d[1]
            for j in range(2, out_order + 1):
                g[j] = d[j - 1] + a * (d[j] - g[j - 1])
        A[:, col] = g
    return A


class MelGeneralizedCepstrumToSpectrum(nn.Module):
    def __init__(self, cep_order, fft_length, alpha=0, gamma=0, out_format="power", n_fft=512, **kwargs):
        super().__init__()
        assert gamma == 0 and out_format == "log-magnitude" and not kwargs, (gamma, out_format, kwargs)
        self.fft_length = fft_length
        self.register_buffer("A", torch.from_numpy(freqt_matrix(cep_order, fft_length // 2, -alpha)))

    def forward(self, mc):
        c = mc @ self.A.t()                                                  # cepstrum on the linear frequency axis
        return torch.fft.rfft(c, n=self.fft_length, dim=-1).real            # zero-padded to fft_length


class MLSA(nn.Module):
    def __init__(self, filter_order, frame_period=None, **kwargs):
        super().__init__()
        self.frame_period = frame_period


_none = lambda *a, **k: None
_mod("pyworld", dio=_none)
_mod("torchlpc", sample_wise_lpc=_none)
_mod("torchaudio")
_mod("torchaudio.functional", lfilter=_none, melscale_fbanks=_none)
_mod("torchaudio.transforms", Spectrogram=Spectrogram, InverseSpectrogram=InverseSpectrogram)
_mod("torch_fftconv")
_mod("torch_fftconv.functional", fft_conv1d=torch.nn.functional.conv1d)
_mod("diffsptk", MLSA=MLSA, MelCepstralAnalysis=_Absent, MelGeneralizedCepstrumToSpectrum=MelGeneralizedCepstrumToSpectrum,
     PQMF=_Absent, IPQMF=_Absent)
_mod("diffsptk.functional", lsp2lpc=_none)

torch.set_default_dtype(torch.float64)
sys.path.insert(0, REF)
import models.utils as ru  # noqa: E402

_mod("models.audiotensor", AudioTensor=ru.LegacyAudioTensor)
import models.filters as rf  # noqa: E402

AT = ru.LegacyAudioTensor
rng = np.random.default_rng(3131)


def g31_filter():
    out = {}
    # F: one control row more than there are frames in case a (an unused row: zero gradient), exactly the frames in case b
    for tag, B, n_fft, hop, T, F in (("a", 2, 256, 64, 6 * 64 + 5, 8), ("b", 1, 1024, 240, 4 * 240 + 17, 5)):
        M, alpha = 24, 0.46
        ex_np = rng.normal(0, 1, (B, T))
        mc_np = rng.normal(0, 1, (B, F, M + 1)) * 0.5 * 0.8 ** np.arange(M + 1)
        mc_np[..., 0] = rng.uniform(-1, 1, (B, F))
        mod = rf.LTVMLSAFilter2(n_fft, hop, M, window="hanning", alpha=alpha, gamma=0)
        ex = torch.tensor(ex_np, requires_grad=True)
        mc = torch.tensor(mc_np, requires_grad=True)
        y = mod(AT(ex), AT(mc, hop_length=hop))
        y = y.as_tensor() if hasattr(y, "as_tensor") else y
        gy = rng.normal(0, 1, tuple(y.shape))
        g_ex, g_mc = torch.autograd.grad((y * torch.as_tensor(gy)).sum(), (ex, mc))
        print(f"g31{tag}: y {tuple(y.shape)} max|y| {float(y.abs().max()):.3f}")
        out.update({f"{tag}_n_fft": n_fft, f"{tag}_hop": hop, f"{tag}_order": M, f"{tag}_alpha": alpha, f"{tag}_ex": ex_np,
                    f"{tag}_mc": mc_np, f"{tag}_y": y.detach().numpy(), f"{tag}_gy": gy, f"{tag}_g_ex": g_ex.numpy(),
                    f"{tag}_g_mc": g_mc.numpy()})
    np.savez_compressed(os.path.join(OUT, "g31_mlsa_filter.npz"), **out)
    print("wrote g31_mlsa_filter.npz:", {k: np.shape(v) for k, v in out.items()})


def g31_config():
    import yaml

    with open(os.path.join(REF, "ckpts", "interspeech24", "mlsa", "config.yaml")) as f:
        model = yaml.safe_load(f)["model"]
    with open(os.path.join(OUT, "g31_mlsa_config.json"), "w") as f:
        json.dump({"model": model}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote g31_mlsa_config.json")


if __name__ == "__main__":
    g31_filter()
    g31_config()
