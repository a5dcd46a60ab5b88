"""CPU: the backward of the STFT-domain frame filter.  The float64 closed form of tests/stft_filter_ref.py (what
golf_stft_filter_frames_bwd_f32 evaluates) against float64 autograd through LTVCepFilter / DiffWorldSPFilter, the argument
checks of the new entry (no launch), and what stays as it was on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import stft_filter_ref as R
from conftest import rel_err

GEOMETRIES = [(64, 24), (128, 32), (128, 50)]   # (n_fft, hop)


def lengths(n, hop):
    """T: a remainder, a multiple of hop (the last frame's reflection reads one sample before its own span), and the shortest
    ones, where one frame reflects at both ends."""
    return [5 * hop + 7, 6 * hop, 2 * hop, n // 2 + 8, n // 2 + 1 + hop]


def make_filter(kind, n, hop):
    from golf_amd.filters import DiffWorldSPFilter, LTVCepFilter

    if kind == "world":
        # f_max above Nyquist: no all-zero column in the rectified pseudo-inverse, whose sqrt has no finite gradient at 0
        return DiffWorldSPFilter(n_mels=12, n_fft=n, hop_length=hop, f_min=0.0, f_max=4400.0, center=True, window="hanning",
                                 sample_rate=8000, norm=None, mel_scale="htk")
    return LTVCepFilter(filter_order=min(24, n // 2 - 1), n_fft=n, window="hanning", hop_length=hop, phase=kind)


def make_ctrl(kind, flt, B, F, gen):
    if kind == "world":
        return torch.exp(0.3 * torch.randn(B, F, 12, generator=gen, dtype=torch.float64) - 2)
    order = flt.filter_order + 1
    return torch.randn(B, F, order, generator=gen, dtype=torch.float64) * 0.2 / (1 + torch.arange(order))


@pytest.mark.parametrize("n,hop", GEOMETRIES)
@pytest.mark.parametrize("kind", ["min", "zero", "world"])
def test_closed_form_is_float64_autograd_through_the_modules(kind, n, hop):
    """Output, d/dx and d/d control (the closed form's response gradient chained to the control input with torch) at 1e-12
    rel-max.  T = 2*hop at (128, 32) is n_fft/2 samples, which cannot be reflect-padded: the module refuses it."""
    from golf_amd.audiotensor import AudioTensor as AT

    gen = torch.Generator().manual_seed(n + hop)
    flt = make_filter(kind, n, hop).double()
    w = flt._window.numpy()
    B = 2
    for T in lengths(n, hop):
        for F in (max(2, T // hop), T // hop + 3):
            x = torch.randn(B, T, generator=gen, dtype=torch.float64, requires_grad=True)
            ctrl = make_ctrl(kind, flt, B, F, gen).requires_grad_()
            if T <= n // 2:
                with pytest.raises(RuntimeError):
                    flt(AT(x), AT(ctrl, hop))
                continue
            y = flt(AT(x), AT(ctrl, hop)).as_tensor()
            gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
            y.backward(gy)
            assert torch.isfinite(ctrl.grad).all()
            c2 = ctrl.detach().clone().requires_grad_()
            H = flt.response_rows(c2)
            assert H.is_complex() == (kind == "min") and H.shape == (B, F, n // 2 + 1)
            Hn = H.detach().numpy()
            yr = R.forward(x.detach().numpy(), Hn, w, hop)
            assert yr.shape == tuple(y.shape) == (B, hop * (min(1 + T // hop, F) - 1))
            gx, gH = R.backward(gy.numpy(), x.detach().numpy(), Hn, w, hop)
            assert gH.dtype == Hn.dtype and not gH[:, min(1 + T // hop, F):].any()
            H.backward(torch.from_numpy(gH))
            for what, got, want in (("y", yr, y.detach()), ("g_x", gx, x.grad), ("g_ctrl", c2.grad, ctrl.grad)):
                e = rel_err(np.asarray(got), want.numpy())[0]
                assert e <= 1e-12, (kind, n, hop, T, F, what, e)


def test_workspace_bytes_of_the_backward():
    from golf_amd import _lib

    wb = _lib.load().golf_stft_filter_frames_bwd_workspace_bytes
    assert wb(2, 200, 7, 64, 24) >= 4 * 2 * 7 * 64 and wb(2, 200, 7, 64, 24) % 256 == 0
    assert wb(2, 200, 20, 64, 24) >= 4 * 2 * 9 * 64             # frames = min(1 + T // hop, F)
    assert wb(2, 200, 7, 96, 24) == 0 and wb(2, 20000, 7, 4096, 240) == 0 and wb(2, 200, 7, 32, 8) == 0
    assert wb(2, 400, 7, 128, 65) == 0 and wb(0, 200, 7, 64, 24) == 0 and wb(2, 200, 0, 64, 24) == 0
    assert wb(2, 32, 7, 64, 24) == 0 and wb(2, 33, 7, 64, 24) > 0   # T <= n_fft/2


def test_backward_entry_refuses_bad_arguments_without_launch():
    from golf_amd import _lib

    lib = _lib.load()
    f = lib.golf_stft_filter_frames_bwd_f32
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    ok = dict(gy=one, gy_stride=144, x=one, x_stride=200, h=one, h_kind=1, window=one, g_x=one, g_x_stride=200, g_h=one, B=2,
              T=200, F=7, n_fft=64, hop=24, ws=one, ws_bytes=1 << 40, stream=None)
    names = list(ok)

    def refused(match, code=-1, **kw):
        rc = f(*[kw.get(k, ok[k]) for k in names])
        assert rc == code, (kw, rc, lib.golf_last_error())
        assert match.encode() in lib.golf_last_error(), (kw, lib.golf_last_error())

    refused("power of two", code=-3, n_fft=96)
    refused("power of two", code=-3, n_fft=4096, T=20000)
    refused("power of two", code=-3, n_fft=32, hop=8)
    refused("< 2*hop", n_fft=128, hop=65, T=400)
    refused("reflect-padded", T=32)
    refused("bad size", B=0)
    refused("bad size", F=0)
    refused("bad size", hop=0)
    refused("bad kind", h_kind=2)
    for k in ("gy", "x", "h", "window"):
        refused("null", **{k: None})
    refused("null", g_x=None, g_h=None)
    refused("stride", gy_stride=143)
    refused("stride", x_stride=199)
    refused("stride", g_x_stride=199)
    need = lib.golf_stft_filter_frames_bwd_workspace_bytes(2, 200, 7, 64, 24)
    refused("workspace", code=-2, ws_bytes=need - 1)
    refused("workspace", code=-2, ws=None)
    refused("workspace", code=-2, ws=ctypes.c_void_p(128))
    # one of the two gradients alone passes the pointer checks (and is then refused on the workspace)
    refused("workspace", code=-2, g_x=None, ws_bytes=0)
    refused("workspace", code=-2, g_h=None, g_x_stride=200, ws_bytes=0)


def test_cpu_tensors_keep_their_paths():
    """The op has no CPU path, with or without grad; the modules run torch.stft / torch.istft on CPU tensors and train there."""
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor as AT

    x = torch.zeros(1, 200, requires_grad=True)
    H, w = torch.ones(1, 7, 33, requires_grad=True), torch.hann_window(64)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.stft_filter_frames(x, H, w, 24)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.stft_filter_frames(x, H.detach().to(torch.complex64).requires_grad_(), w, 24)
    with pytest.raises(GolfError, match="reflect-padded"):
        GF.stft_filter_frames(x[:, :32], H, w, 24)
    gen = torch.Generator().manual_seed(5)
    for kind in ("min", "zero", "world"):
        flt = make_filter(kind, 128, 32)
        assert flt.hip_frames is True
        x = torch.randn(2, 300, generator=gen, requires_grad=True)
        ctrl = make_ctrl(kind, flt, 2, 9, gen).float().requires_grad_()
        y = flt(AT(x), AT(ctrl, 32)).as_tensor()
        assert y.shape == (2, 32 * 8)
        y.square().sum().backward()
        assert torch.isfinite(x.grad).all() and torch.isfinite(ctrl.grad).all() and ctrl.grad.abs().max() > 0
